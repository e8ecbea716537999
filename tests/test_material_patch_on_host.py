"""The per-thread work of the in-place material update (csrc/device/material_patch.h: patchMaterialSlot of k_patch_materials) compiled for the
host through tests/host_shim -- no GPU needed.  A small triangle array is built by worldTriangle + makeAlphaRecord under OLD tables and flags,
patched under NEW ones, and must then equal, byte for byte, the array the same two functions build under the new tables: for each dirty-bit
combination, with the opaque-triangle prefix of a cut primitive, a clean render node left untouched, and pre-split references (several slots
of one triangle)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vk_gltf_renderer_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPAQUE, MASK, BLEND = 0, 1, 2
FORCE_OPAQUE, CULL_DISABLE, FLIP, TRANSMISSIVE, ALPHA_PASSES = 1, 2, 4, 8, 16
PATCH_FLAGS, PATCH_ALPHA = 1, 2
NUM_NODES = 5


class ShimPrim(C.Structure):
    _fields_ = [("indices", C.c_void_p), ("positions", C.c_void_p), ("colors", C.c_void_p), ("texCoords0", C.c_void_p), ("texCoords1", C.c_void_p),
                ("opaqueTriangles", C.c_uint32), ("pad", C.c_uint32)]


class ShimTexture(C.Structure):
    _fields_ = [("level0", C.c_uint32), ("width", C.c_uint16), ("height", C.c_uint16), ("magFilter", C.c_uint8), ("wrapS", C.c_uint8), ("wrapT", C.c_uint8),
                ("pad", C.c_uint8)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_shim_material_patch") / "libmaterial_patch_on_host.so")
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + shim, "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"),
                    "-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(shim, "material_patch_on_host.cpp")], check=True)
    L = C.CDLL(out)
    VP, I, U = C.c_void_p, C.c_int, C.c_uint32
    L.patch_build.argtypes = [VP, I, VP, I, VP, I, VP, VP, I, VP, VP, VP, U, VP, VP]
    L.patch_slots.argtypes = [VP, I, VP, I, VP, I, VP, VP, I, VP, VP, U, VP, VP]
    return L


def ptr(a):
    return a.ctypes.data


class World:
    """Five render nodes over two primitives (primitive 1 was cut at load: its first 7 triangles are opaque), three materials, two textures;
    node 4 shares material 1 with node 1.  Slots: every triangle of every node once, a few of them three times (pre-split references),
    shuffled like a tree's order."""

    def __init__(self, seed=0):
        rng = np.random.default_rng(seed)
        self.keep = []
        self.prims = (ShimPrim * 2)()
        self.tri_count = [23, 19]
        for p, nt in enumerate(self.tri_count):
            pos = rng.normal(size=(nt * 3, 3)).astype(np.float32)
            idx = rng.permutation(nt * 3).astype(np.uint32)
            uv0 = rng.uniform(-1, 2, (nt * 3, 2)).astype(np.float32)
            uv1 = rng.uniform(-1, 2, (nt * 3, 2)).astype(np.float32)
            col = rng.integers(0, 2 ** 32, nt * 3, dtype=np.uint64).astype(np.uint32)
            self.keep += [pos, idx, uv0, uv1, col]
            self.prims[p].indices, self.prims[p].positions, self.prims[p].texCoords0, self.prims[p].texCoords1 = ptr(idx), ptr(pos), ptr(uv0), ptr(uv1)
            self.prims[p].colors = ptr(col) if p == 0 else None
            self.prims[p].opaqueTriangles = 7 if p == 1 else 0
        self.node_prim = [0, 1, 0, 1, 1]
        self.node_mat = [0, 1, 2, 0, 1]
        self.nodes = (capi.MiGltfRenderNode * NUM_NODES)()
        for n in range(NUM_NODES):
            M = np.eye(4)
            M[:3, :3] = rng.normal(size=(3, 3))
            M[:3, 3] = rng.normal(size=3)
            self.nodes[n].objectToWorld[:] = [float(v) for v in M.T.reshape(-1).astype(np.float32)]
            self.nodes[n].worldToObject[:] = [float(v) for v in np.linalg.inv(M).T.reshape(-1).astype(np.float32)]
            self.nodes[n].renderPrimID, self.nodes[n].materialID = self.node_prim[n], self.node_mat[n]
        self.textures = (ShimTexture * 2)()
        self.textures[0].level0, self.textures[0].width, self.textures[0].height, self.textures[0].magFilter, self.textures[0].wrapS = 0, 8, 4, 1, 1
        self.textures[1].level0, self.textures[1].width, self.textures[1].height, self.textures[1].wrapT = 32, 16, 16, 2
        slots = []
        for n in range(NUM_NODES):
            for t in range(self.tri_count[self.node_prim[n]]):
                slots += [(n, t)] * (3 if (t % 6 == 5) else 1)
        order = rng.permutation(len(slots))
        self.slot_node = np.array([slots[i][0] for i in order], np.int32)
        self.slot_tri = np.array([slots[i][1] for i in order], np.uint32)
        assert len(order) > 100 and len(order) % 64 != 0

    def tables(self, edits=()):
        """Three materials and four texture infos (slot 0 reserved); `edits`: functions of (materials, infos)."""
        mats = (capi.MiGltfShadeMaterial * 3)()
        infos = (capi.MiGltfTextureInfo * 4)()
        for i in range(4):
            infos[i].uvTransform[:] = [1, 0, 0, 1, 0, 0]
            infos[i].index, infos[i].texCoord = [-1, 0, 1, 0][i], [0, 0, 1, 1][i]
        for m in range(3):
            mats[m].pbrBaseColorFactor[:] = [0.8, 0.7, 0.6, 1.0]
            mats[m].pbrDiffuseFactor[:] = [0.5, 0.5, 0.5, 0.25]
            mats[m].alphaCutoff = 0.5
        mats[1].alphaMode, mats[1].pbrBaseColorTexture = MASK, 1
        mats[2].alphaMode, mats[2].pbrBaseColorFactor[3] = BLEND, 0.4
        for e in edits:
            e(mats, infos)
        return mats, infos

    def build(self, lib, mats, infos, flags):
        n = len(self.slot_node)
        tris, alpha = np.zeros((n, 12), np.uint32), np.zeros((n, 12), np.uint32)
        lib.patch_build(C.addressof(self.nodes), NUM_NODES, C.addressof(self.prims), 2, C.addressof(mats), 3, C.addressof(infos), C.addressof(self.textures), 2,
                        ptr(flags), ptr(self.slot_node), ptr(self.slot_tri), n, ptr(tris), ptr(alpha))
        return tris, alpha

    def patch(self, lib, mats, infos, flags, dirty, tris, alpha):
        lib.patch_slots(C.addressof(self.nodes), NUM_NODES, C.addressof(self.prims), 2, C.addressof(mats), 3, C.addressof(infos), C.addressof(self.textures), 2,
                        ptr(flags), ptr(dirty), len(self.slot_node), ptr(tris), ptr(alpha) if alpha is not None else None)


def _inst_flags(world, mat_flags, flip=(2,)):
    return np.array([mat_flags[world.node_mat[n]] | (FLIP if n in flip else 0) for n in range(NUM_NODES)], np.uint8)


OLD_FLAGS = [FORCE_OPAQUE, 0, CULL_DISABLE]
# the new state: material 0 turns transmissive and double sided (flags only), material 1 gets another cutoff, texture and texture set
# (alpha only), material 2 goes BLEND -> MASK on the specular-glossiness model, single sided (both)
NEW_FLAGS = [CULL_DISABLE | TRANSMISSIVE | ALPHA_PASSES, 0, 0]


def _edit(mats, infos):
    mats[0].transmissionFactor, mats[0].doubleSided = 0.5, 1
    mats[1].alphaCutoff, mats[1].pbrBaseColorTexture = 0.25, 2
    mats[2].alphaMode, mats[2].pbrModel, mats[2].pbrDiffuseTexture = MASK, 1, 3


def test_patched_slots_equal_a_build_under_the_new_tables(lib):
    w = World()
    old_m, old_i = w.tables()
    new_m, new_i = w.tables([_edit])
    tris, alpha = w.build(lib, old_m, old_i, _inst_flags(w, OLD_FLAGS))
    want_tris, want_alpha = w.build(lib, new_m, new_i, _inst_flags(w, NEW_FLAGS))
    assert tris.tobytes() != want_tris.tobytes() and alpha.tobytes() != want_alpha.tobytes()
    # nodes 0, 3: material 0 (flags); nodes 1, 4: material 1 (alpha); node 2: material 2 (both)
    dirty = np.array([PATCH_FLAGS, PATCH_ALPHA, PATCH_FLAGS | PATCH_ALPHA, PATCH_FLAGS, PATCH_ALPHA], np.uint8)
    w.patch(lib, new_m, new_i, _inst_flags(w, NEW_FLAGS), dirty, tris, alpha)
    assert tris.tobytes() == want_tris.tobytes()
    assert alpha.tobytes() == want_alpha.tobytes()
    # the flag word alone moved in the triangle records
    before, _ = w.build(lib, old_m, old_i, _inst_flags(w, OLD_FLAGS))
    assert (before[:, :11] == tris[:, :11]).all()


def test_each_dirty_bit_touches_its_own_record_only(lib):
    w = World(1)
    old_m, old_i = w.tables()
    new_m, new_i = w.tables([_edit])
    old_f, new_f = _inst_flags(w, OLD_FLAGS), _inst_flags(w, NEW_FLAGS)
    old_tris, old_alpha = w.build(lib, old_m, old_i, old_f)
    new_tris, new_alpha = w.build(lib, new_m, new_i, new_f)
    for bits in (0, PATCH_FLAGS, PATCH_ALPHA, PATCH_FLAGS | PATCH_ALPHA):
        for node in range(NUM_NODES):
            tris, alpha = old_tris.copy(), old_alpha.copy()
            dirty = np.zeros(NUM_NODES, np.uint8)
            dirty[node] = bits
            w.patch(lib, new_m, new_i, new_f, dirty, tris, alpha)
            mine = w.slot_node == node
            assert (tris[~mine] == old_tris[~mine]).all() and (alpha[~mine] == old_alpha[~mine]).all(), (bits, node)  # a clean node's slots stay
            assert (tris[mine] == (new_tris if bits & PATCH_FLAGS else old_tris)[mine]).all(), (bits, node)
            assert (alpha[mine] == (new_alpha if bits & PATCH_ALPHA else old_alpha)[mine]).all(), (bits, node)


def test_opaque_prefix_of_a_cut_primitive_keeps_force_opaque(lib):
    w = World(2)
    mats, infos = w.tables()
    tris, alpha = w.build(lib, mats, infos, _inst_flags(w, OLD_FLAGS))
    new_f = _inst_flags(w, [0, CULL_DISABLE, 0])
    w.patch(lib, mats, infos, new_f, np.full(NUM_NODES, PATCH_FLAGS, np.uint8), tris, None)  # (no alpha records: the alpha bit has nothing to write)
    word = tris[:, 11]
    for n in range(NUM_NODES):
        mine = w.slot_node == n
        cut = mine & (w.slot_tri < 7) & (w.node_prim[n] == 1)
        assert (word[mine & ~cut] == new_f[n]).all(), n
        assert (word[cut] == (new_f[n] | FORCE_OPAQUE)).all(), n
    assert ((w.slot_tri < 7) & (np.array(w.node_prim)[w.slot_node] == 1)).sum() >= 21
    want, _ = w.build(lib, mats, infos, new_f)
    assert tris.tobytes() == want.tobytes()


def test_split_references_of_one_triangle_all_get_the_patch(lib):
    w = World(3)
    old_m, old_i = w.tables()
    new_m, new_i = w.tables([_edit])
    tris, alpha = w.build(lib, old_m, old_i, _inst_flags(w, OLD_FLAGS))
    w.patch(lib, new_m, new_i, _inst_flags(w, NEW_FLAGS), np.full(NUM_NODES, PATCH_FLAGS | PATCH_ALPHA, np.uint8), tris, alpha)
    key = w.slot_node.astype(np.int64) * 1000 + w.slot_tri
    groups = 0
    for k in np.unique(key):
        s = np.flatnonzero(key == k)
        if len(s) > 1:
            groups += 1
            assert (tris[s] == tris[s[0]]).all() and (alpha[s] == alpha[s[0]]).all()
    assert groups > 10
