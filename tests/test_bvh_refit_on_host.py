"""The per-thread work of the 8-wide BVH refit (csrc/device/bvh_refit.h: refitTriSlot of k_refit_tris, refitNode8 of k_refit_level, the
quantisation shared with k_collapse_emit) compiled for the host through tests/host_shim -- no GPU needed.  On random small trees: every
decoded child box contains the triangles below it after random moves; a refit with nothing moved reproduces the builder's node bytes; a
refit to a pose after other poses equals a refit straight to it; a moved pre-split reference gets its triangle's box, one back home the
box it was built with."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vk_gltf_renderer_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE8 = np.dtype([("p", "<f4", 3), ("e", "u1", 3), ("imask", "u1"), ("childBase", "<u4"), ("triBase", "<u4"), ("valid", "<u2"),
                  ("r16", "<u2"), ("r32", "<u4"), ("qlo", "u1", (3, 8)), ("qhi", "u1", (3, 8))])
assert NODE8.itemsize == 80
MOVED, HOME = 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_shim_refit") / "librefit_on_host.so")
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + shim, "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"),
                    "-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(shim, "refit_on_host.cpp")], check=True)
    L = C.CDLL(out)
    VP = C.c_void_p
    L.refit_quantise.argtypes = [VP, VP, VP, VP, VP, C.c_uint32]
    L.refit_levels.argtypes = [VP, VP, C.c_int, VP, VP, VP]
    L.refit_tris.argtypes = [VP, VP, VP, C.c_uint32, VP, VP, VP, VP, VP, C.c_uint32]
    return L


def ptr(a):
    return a.ctypes.data


class Tree:
    """A random 8-wide tree in the layout of bvh8.hip: breadth-first levels, inner children contiguous from childBase and leaf triangles
    contiguous from triBase, both in slot order; leaf children of one or two triangles; render nodes own runs of triangles."""

    def __init__(self, rng, num_tris=300, num_nodes=5):
        self.rng = rng
        self.num_nodes = num_nodes
        self.tri_node = np.sort(rng.integers(0, num_nodes, num_tris))  # render node of each scene triangle
        self.tri_index = np.arange(num_tris, dtype=np.uint32)           # its triangle index in the (shared) primitive
        nodes, levels, slots = [], [0], []
        level = [list(rng.permutation(num_tris))]
        while level:
            nxt = []
            for tris in level:
                k = int(rng.integers(2, 9))
                cuts = np.sort(rng.choice(np.arange(1, len(tris)), size=min(k, len(tris)) - 1, replace=False)) if len(tris) > 1 else []
                groups = [g for g in np.split(np.array(tris), cuts) if len(g)]
                slot_of = rng.permutation(8)[:len(groups)]
                n = np.zeros((), NODE8)
                n["childBase"] = levels[-1] + len(level) + len(nxt)
                n["triBase"] = 0  # patched below (leaf triangles are appended level by level, in node order)
                children = sorted(zip(slot_of, groups), key=lambda sg: sg[0])
                leaf_tris, imask, valid = [], 0, 0
                for sl, g in children:
                    if len(g) <= 2:
                        valid |= (3 if len(g) == 2 else 1) << (2 * int(sl))
                        leaf_tris.extend(int(t) for t in g)
                    else:
                        imask |= 1 << int(sl)
                        nxt.append(list(g))
                n["imask"], n["valid"] = imask, valid
                nodes.append((n, leaf_tris, children))
            levels.append(len(nodes))
            level = nxt
        self.levels = np.array(levels, np.uint32)
        self.nodes = np.zeros(len(nodes), NODE8)
        order = []
        for i, (n, leaf_tris, children) in enumerate(nodes):
            n["triBase"] = len(order)
            order.extend(leaf_tris)
            self.nodes[i] = n
        self.children = [c for _, _, c in nodes]
        self.order = np.array(order)  # slot -> scene triangle
        self.slot_node = self.tri_node[self.order].astype(np.int32)


def render_nodes(mats):
    arr = (capi.MiGltfRenderNode * len(mats))()
    for i, M in enumerate(mats):
        arr[i].objectToWorld[:] = [float(v) for v in np.asarray(M, np.float32).T.reshape(-1)]
        arr[i].worldToObject[:] = [float(v) for v in np.linalg.inv(np.asarray(M, np.float64)).astype(np.float32).T.reshape(-1)]
        arr[i].renderPrimID, arr[i].materialID = 0, 0
    return arr


def random_pose(rng, n):
    mats = []
    for _ in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        M = np.eye(4)
        M[:3, :3] = R * rng.uniform(0.5, 2.0)
        M[:3, 3] = rng.normal(size=3) * 3.0
        mats.append(M)
    return mats


class Scene:
    def __init__(self, lib, seed):
        self.lib = lib
        rng = np.random.default_rng(seed)
        self.rng = rng
        self.tree = Tree(rng)
        nt = len(self.tree.order)
        centres = rng.normal(size=(nt, 3)) * 2.0
        self.positions = (centres[:, None, :] + rng.normal(size=(nt, 3, 3)) * 0.2).astype(np.float32).reshape(-1, 3)
        self.indices = np.arange(nt * 3, dtype=np.uint32)
        self.flags = np.zeros(self.tree.num_nodes, np.uint8)
        # the slots' triangle records: render node (a.w) and triangle index (b.w) are all k_refit_tris reads from them
        self.tris = np.zeros((nt, 12), np.float32)
        self.tris[:, 3] = self.tree.slot_node.view(np.float32)
        self.tris[:, 7] = self.tree.tri_index[self.tree.order].view(np.float32)
        self.slot_box = np.zeros((nt, 6), np.float32)

    def pose_tris(self, mats, dirty, built_box=None):
        """k_refit_tris for the render nodes whose byte in `dirty` is set; returns the slot boxes."""
        nodes = render_nodes(mats)
        built = built_box if built_box is not None else self.slot_box
        self.lib.refit_tris(C.addressof(nodes), ptr(self.indices), ptr(self.positions), 0, ptr(self.flags), ptr(np.asarray(dirty, np.uint8)), ptr(built),
                            ptr(self.tris), ptr(self.slot_box), len(self.tris))
        return self.slot_box.copy()

    def build(self, mats):
        """The builder's side: slot boxes of the pose, child boxes as exact unions in numpy, quantised by the builder's function."""
        self.pose_tris(mats, np.full(self.tree.num_nodes, MOVED))
        built = self.slot_box.copy()
        out = self.tree.nodes.copy()
        nb = np.zeros((len(out), 6), np.float32)
        for i in reversed(range(len(out))):
            clo, chi, used = np.zeros((3, 8), np.float32), np.zeros((3, 8), np.float32), 0
            child, tri = int(out[i]["childBase"]), int(out[i]["triBase"])
            for sl in range(8):
                v = (int(out[i]["valid"]) >> (2 * sl)) & 3
                if (int(out[i]["imask"]) >> sl) & 1:
                    b = nb[child]
                    child += 1
                elif v:
                    cnt = 2 if v & 2 else 1
                    b = np.concatenate([built[tri:tri + cnt, :3].min(0), built[tri:tri + cnt, 3:].max(0)])
                    tri += cnt
                else:
                    continue
                clo[:, sl], chi[:, sl] = b[:3], b[3:]
                used |= 1 << sl
            lo = clo[:, [s for s in range(8) if used >> s & 1]].min(1)
            hi = chi[:, [s for s in range(8) if used >> s & 1]].max(1)
            nb[i] = np.concatenate([lo, hi])
            self.lib.refit_quantise(out[i:i + 1].ctypes.data, ptr(lo), ptr(hi), ptr(clo), ptr(chi), used)
        return out, built

    def refit(self, nodes8):
        nodes8 = nodes8.copy()
        nb = np.zeros((len(nodes8), 6), np.float32)
        sah = np.zeros(len(nodes8), np.float32)
        self.lib.refit_levels(nodes8.ctypes.data, ptr(self.tree.levels), len(self.tree.levels) - 1, ptr(self.slot_box), ptr(nb), ptr(sah))
        return nodes8, sah


def decode(node, sl):
    scale = np.ldexp(np.float32(1), node["e"].astype(np.int32) - 127).astype(np.float64)
    p = node["p"].astype(np.float64)
    lo = (node["qlo"][:, sl].astype(np.float64) * scale + p).astype(np.float32)
    hi = (node["qhi"][:, sl].astype(np.float64) * scale + p).astype(np.float32)
    return lo, hi


def world_vertices(sc, mats, slots):
    out = []
    for s in slots:
        M = np.asarray(mats[int(sc.tree.slot_node[s])], np.float64)
        t = int(sc.tree.order[s])
        v = sc.positions[3 * t:3 * t + 3].astype(np.float64)
        out.append(v @ M[:3, :3].T + M[:3, 3])
    return np.concatenate(out)


def check_contains(sc, nodes8, mats):
    slots_below = {}
    for i in reversed(range(len(nodes8))):
        n = nodes8[i]
        child, tri, below = int(n["childBase"]), int(n["triBase"]), []
        for sl in range(8):
            v = (int(n["valid"]) >> (2 * sl)) & 3
            if (int(n["imask"]) >> sl) & 1:
                slots = slots_below[child]
                child += 1
            elif v:
                cnt = 2 if v & 2 else 1
                slots = list(range(tri, tri + cnt))
                tri += cnt
            else:
                continue
            below += slots
            lo, hi = decode(n, sl)
            w = world_vertices(sc, mats, slots)
            tol = 1e-5 * (1 + np.abs(w))  # (the vertices here are float64 products; the device's are float32 fmaf chains)
            assert (w >= lo - tol).all() and (w <= hi + tol).all(), (i, sl)
        slots_below[i] = below


def test_refit_with_nothing_moved_reproduces_the_node_bytes(lib):
    for seed in range(6):
        sc = Scene(lib, seed)
        mats = random_pose(sc.rng, sc.tree.num_nodes)
        built, _ = sc.build(mats)
        again, sah = sc.refit(built)
        assert again.tobytes() == built.tobytes(), seed
        assert (sah > 0).all()


def test_decoded_boxes_contain_their_triangles_after_random_moves(lib):
    for seed in range(6):
        sc = Scene(lib, 100 + seed)
        mats = random_pose(sc.rng, sc.tree.num_nodes)
        built, _ = sc.build(mats)
        nodes8 = built
        for step in range(4):
            moved = sc.rng.random(sc.tree.num_nodes) < 0.6
            new = random_pose(sc.rng, sc.tree.num_nodes)
            mats = [new[i] if moved[i] else mats[i] for i in range(len(mats))]
            sc.pose_tris(mats, moved.astype(np.uint8) * MOVED)
            nodes8, _ = sc.refit(nodes8)
            check_contains(sc, nodes8, mats)
        # the slot assignment and the tree's links stay
        for f in ("childBase", "triBase", "valid", "imask"):
            assert (nodes8[f] == built[f]).all()


def test_refit_depends_on_the_current_pose_only(lib):
    sc = Scene(lib, 7)
    m0 = random_pose(sc.rng, sc.tree.num_nodes)
    built, _ = sc.build(m0)
    poses = [random_pose(sc.rng, sc.tree.num_nodes) for _ in range(4)]
    n = sc.tree.num_nodes
    # straight to P
    sc.pose_tris(poses[3], np.full(n, MOVED))
    direct, sah_direct = sc.refit(built)
    tris_direct = sc.tris.copy()
    # A, B, C, then P, each step moving only the nodes that changed
    sc2 = Scene(lib, 7)
    _, built_box = sc2.build(m0)
    nodes8 = built
    for P in poses:
        sc2.pose_tris(P, np.full(n, MOVED))
        nodes8, sah = sc2.refit(nodes8)
    assert nodes8.tobytes() == direct.tobytes()
    assert sah.tobytes() == sah_direct.tobytes()
    assert sc2.tris.tobytes() == tris_direct.tobytes()
    # and back to the build's pose: the built bytes again
    sc2.pose_tris(m0, np.full(n, HOME), built_box=built_box)
    back, _ = sc2.refit(nodes8)
    assert back.tobytes() == built.tobytes()


def test_moved_split_reference_gets_its_triangles_box(lib):
    sc = Scene(lib, 11)
    mats = random_pose(sc.rng, sc.tree.num_nodes)
    _, built = sc.build(mats)
    whole = built.copy()
    # a pre-split reference was filed under a clipped (smaller) box
    clipped = built.copy()
    s = 5
    mid = 0.5 * (whole[s, :3] + whole[s, 3:])
    clipped[s, 3:] = mid
    sc.slot_box[:] = clipped
    dirty = np.zeros(sc.tree.num_nodes, np.uint8)
    dirty[sc.tree.slot_node[s]] = MOVED
    got = sc.pose_tris(mats, dirty, built_box=clipped)
    assert (got[s] == whole[s]).all()  # moved: the whole triangle's box (it covers every reference of the triangle)
    dirty[sc.tree.slot_node[s]] = HOME
    got = sc.pose_tris(mats, dirty, built_box=clipped)
    assert (got[s] == clipped[s]).all()  # back home: the box it was built with
    other = sc.tree.slot_node != sc.tree.slot_node[s]
    assert (got[other] == clipped[other]).all()  # clean slots keep their boxes
