"""The per-thread work of resident mode (mi_pt_set_accel_resident) compiled for the host through tests/host_shim -- no GPU needed: the refit
with hidden slots (csrc/device/bvh_refit.h: REFIT_HIDDEN of refitTriSlot, emptiness in refitNode8) on the random small trees of
test_bvh_refit_on_host.py (300 triangles, 5 render nodes), and the material patch with shade records (csrc/device/material_patch.h:
MATERIAL_PATCH_SHADE) on the small world of test_material_patch_on_host.py.

Hidden slots: after hiding random subsets of the render nodes every decoded box of a non-empty child contains the visible triangles below
it, every child with nothing visible below it holds the inverted bytes 255 / 0, every Node8::p and every SAH term is finite; hide followed by
show gives back the built node bytes and slot boxes exactly; hide, move, show equals a plain move; a two-triangle leaf with one hidden
triangle gets the other's box; an all-hidden tree reports an empty root.  Shade patch: a patched slot holds the materialID a build writes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_bvh_refit_on_host import HOME, MOVED, Scene, decode, random_pose, world_vertices
from test_material_patch_on_host import (CULL_DISABLE, FORCE_OPAQUE, NUM_NODES, PATCH_ALPHA, PATCH_FLAGS, TRANSMISSIVE, ALPHA_PASSES, World,
                                         _inst_flags)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN = 3
PATCH_SHADE = 4
FLT_MAX = np.float32(3.4028234663852886e38)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_shim_resident") / "libresident_on_host.so")
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + shim, "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"),
                    "-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(shim, "resident_on_host.cpp")], check=True)
    L = C.CDLL(out)
    VP, I, U = C.c_void_p, C.c_int, C.c_uint32
    L.refit_quantise.argtypes = [VP, VP, VP, VP, VP, U]
    L.refit_levels.argtypes = [VP, VP, I, VP, VP, VP]
    L.refit_tris.argtypes = [VP, VP, VP, U, VP, VP, VP, VP, VP, U]
    L.resident_build.argtypes = [VP, I, VP, I, VP, I, VP, VP, I, VP, VP, VP, U, VP, VP, VP]
    L.resident_patch.argtypes = [VP, I, VP, I, VP, I, VP, VP, I, VP, VP, U, VP, VP, VP]
    return L


def ptr(a):
    return a.ctypes.data


def refit_with_boxes(sc, nodes8):
    """Scene.refit, returning the node boxes too."""
    nodes8 = nodes8.copy()
    nb = np.zeros((len(nodes8), 6), np.float32)
    sah = np.zeros(len(nodes8), np.float32)
    sc.lib.refit_levels(nodes8.ctypes.data, ptr(sc.tree.levels), len(sc.tree.levels) - 1, ptr(sc.slot_box), ptr(nb), ptr(sah))
    return nodes8, sah, nb


def children(n):
    """(slot, is inner, first index, count) of the children of a node, in slot order."""
    child, tri = int(n["childBase"]), int(n["triBase"])
    for sl in range(8):
        v = (int(n["valid"]) >> (2 * sl)) & 3
        if (int(n["imask"]) >> sl) & 1:
            yield sl, True, child, 1
            child += 1
        elif v:
            cnt = 2 if v & 2 else 1
            yield sl, False, tri, cnt
            tri += cnt


def check_hidden_tree(sc, nodes8, mats, visible):
    """Containment of what is visible, inverted bytes for what is not, finite planes.  Returns the visible slots below every node."""
    below_all = {}
    for i in reversed(range(len(nodes8))):
        n = nodes8[i]
        assert np.isfinite(n["p"]).all() and (np.abs(n["p"]) < 1e30).all(), i
        below = []
        for sl, inner, first, cnt in children(n):
            slots = below_all[first] if inner else [s for s in range(first, first + cnt) if visible[sc.tree.slot_node[s]]]
            below += slots
            if not slots:  # nothing visible below: the inverted box of an empty slot on every axis
                assert (n["qlo"][:, sl] == 255).all() and (n["qhi"][:, sl] == 0).all(), (i, sl)
                continue
            lo, hi = decode(n, sl)
            w = world_vertices(sc, mats, slots)
            tol = 1e-5 * (1 + np.abs(w))
            assert (w >= lo - tol).all() and (w <= hi + tol).all(), (i, sl)
            assert (n["qlo"][:, sl] <= n["qhi"][:, sl]).all(), (i, sl)
        below_all[i] = below
    return below_all


def hide(sc, mats, hidden_nodes):
    dirty = np.zeros(sc.tree.num_nodes, np.uint8)
    dirty[list(hidden_nodes)] = HIDDEN
    return sc.pose_tris(mats, dirty)


def test_hidden_subsets_keep_the_visible_triangles_and_invert_the_rest(lib):
    fully_hidden_children = 0
    for seed in range(6):
        sc = Scene(lib, 300 + seed)
        n = sc.tree.num_nodes
        mats = random_pose(sc.rng, n)
        built, built_box = sc.build(mats)
        nodes8 = built
        visible = np.ones(n, bool)
        for step in range(4):
            now = sc.rng.random(n) < 0.5
            dirty = np.zeros(n, np.uint8)
            dirty[visible & ~now] = HIDDEN
            dirty[~visible & now] = HOME
            sc.pose_tris(mats, dirty, built_box=built_box)
            visible = now
            nodes8, sah, nb = refit_with_boxes(sc, nodes8)
            assert np.isfinite(sah).all() and (sah >= 0).all()
            below = check_hidden_tree(sc, nodes8, mats, visible)
            fully_hidden_children += sum(1 for i in below if i and not below[i])
            # hidden slots: a point at the origin that keeps render node, triangle index and flag word; an empty box
            hid = ~visible[sc.tree.slot_node]
            assert (sc.tris[hid][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] == 0).all()
            assert (sc.tris[:, 3].view(np.int32) == sc.tree.slot_node).all()
            assert (sc.tris[:, 7].view(np.uint32) == sc.tree.tri_index[sc.tree.order]).all()
            assert (sc.slot_box[hid, :3] == FLT_MAX).all() and (sc.slot_box[hid, 3:] == -FLT_MAX).all()
            # an inner node's own box is empty exactly when nothing below it is visible
            for i in range(len(nodes8)):
                assert (nb[i, 0] > nb[i, 3]) == (not below[i]), i
        for f in ("childBase", "triBase", "valid", "imask"):
            assert (nodes8[f] == built[f]).all()
    assert fully_hidden_children > 0  # (the case occurred: inner children with nothing visible below them)


def test_hide_then_show_reproduces_the_built_bytes(lib):
    for seed in range(4):
        sc = Scene(lib, 400 + seed)
        n = sc.tree.num_nodes
        mats = random_pose(sc.rng, n)
        built, built_box = sc.build(mats)
        tris_built = sc.tris.copy()
        hidden = np.flatnonzero(sc.rng.random(n) < 0.6)
        hide(sc, mats, hidden)
        nodes8, _, _ = refit_with_boxes(sc, built)
        assert len(hidden) == 0 or nodes8.tobytes() != built.tobytes()
        dirty = np.zeros(n, np.uint8)
        dirty[hidden] = HOME
        boxes = sc.pose_tris(mats, dirty, built_box=built_box)
        back, sah, _ = refit_with_boxes(sc, nodes8)
        assert back.tobytes() == built.tobytes(), seed
        assert boxes.tobytes() == built_box.tobytes(), seed
        assert sc.tris.tobytes() == tris_built.tobytes(), seed
        _, sah_built, _ = refit_with_boxes(sc, built)
        assert sah.tobytes() == sah_built.tobytes()


def test_hide_move_show_equals_a_plain_move(lib):
    sc = Scene(lib, 17)
    n = sc.tree.num_nodes
    m0, m1 = random_pose(sc.rng, n), random_pose(sc.rng, n)
    built, _ = sc.build(m0)
    sc.pose_tris(m1, np.full(n, MOVED))
    want, want_sah, _ = refit_with_boxes(sc, built)
    want_tris, want_boxes = sc.tris.copy(), sc.slot_box.copy()
    # the same tree: nodes 1 and 3 hidden, every node moved while they are hidden (hidden ones stay clean), then shown
    sc2 = Scene(lib, 17)
    sc2.build(m0)
    hide(sc2, m0, [1, 3])
    nodes8, _, _ = refit_with_boxes(sc2, built)
    dirty = np.full(n, MOVED, np.uint8)
    dirty[[1, 3]] = 0
    sc2.pose_tris(m1, dirty)
    nodes8, _, _ = refit_with_boxes(sc2, nodes8)
    check_hidden_tree(sc2, nodes8, m1, np.array([True, False, True, False, True]))
    dirty = np.zeros(n, np.uint8)
    dirty[[1, 3]] = MOVED
    sc2.pose_tris(m1, dirty)
    got, got_sah, _ = refit_with_boxes(sc2, nodes8)
    assert got.tobytes() == want.tobytes()
    assert got_sah.tobytes() == want_sah.tobytes()
    assert sc2.tris.tobytes() == want_tris.tobytes() and sc2.slot_box.tobytes() == want_boxes.tobytes()


def test_two_triangle_leaf_with_one_hidden_triangle_gets_the_others_box(lib):
    checked = 0
    for seed in range(4):
        sc = Scene(lib, 500 + seed)
        n = sc.tree.num_nodes
        mats = random_pose(sc.rng, n)
        built, built_box = sc.build(mats)
        hide(sc, mats, [2])
        nodes8, _, _ = refit_with_boxes(sc, built)
        for i, node in enumerate(nodes8):
            for sl, inner, first, cnt in children(node):
                if inner or cnt != 2:
                    continue
                a, b = (sc.tree.slot_node[first] == 2), (sc.tree.slot_node[first + 1] == 2)
                if a == b:
                    continue
                other = first + 1 if a else first
                # the child's box is the visible triangle's alone: quantising that box in the node's frame gives the same bytes
                lo, hi = decode(node, sl)
                scale = np.ldexp(np.float32(1), node["e"].astype(np.int32) - 127)
                assert (lo <= built_box[other, :3]).all() and (hi >= built_box[other, 3:]).all()
                assert (lo > built_box[other, :3] - 2.0 * scale).all() and (hi < built_box[other, 3:] + 2.0 * scale).all(), (i, sl)
                checked += 1
    assert checked > 5


def test_all_hidden_tree_reports_an_empty_root(lib):
    sc = Scene(lib, 23)
    n = sc.tree.num_nodes
    mats = random_pose(sc.rng, n)
    built, built_box = sc.build(mats)
    hide(sc, mats, range(n))
    nodes8, sah, nb = refit_with_boxes(sc, built)
    assert (nb[:, :3] == FLT_MAX).all() and (nb[:, 3:] == -FLT_MAX).all()
    assert (sah == 0).all()
    assert (nodes8["qlo"] == 255).all() and (nodes8["qhi"] == 0).all()
    assert (nodes8["p"] == built["p"]).all()  # the planes the walks subtract the origin from stay where they were: finite
    for f in ("childBase", "triBase", "valid", "imask"):
        assert (nodes8[f] == built[f]).all()
    # ... a second refit of the all-hidden tree changes nothing, and showing everything gives the built tree back
    again, _, _ = refit_with_boxes(sc, nodes8)
    assert again.tobytes() == nodes8.tobytes()
    sc.pose_tris(mats, np.full(n, HOME, np.uint8), built_box=built_box)
    back, _, _ = refit_with_boxes(sc, nodes8)
    assert back.tobytes() == built.tobytes()


# ---- the shade-record patch ------------------------------------------------------------------------------------------------------------
def _build(w, lib, mats, infos, flags):
    n = len(w.slot_node)
    tris, alpha, shade = np.zeros((n, 12), np.uint32), np.zeros((n, 12), np.uint32), np.zeros((n, 8), np.uint32)
    lib.resident_build(C.addressof(w.nodes), NUM_NODES, C.addressof(w.prims), 2, C.addressof(mats), 3, C.addressof(infos), C.addressof(w.textures), 2,
                       ptr(flags), ptr(w.slot_node), ptr(w.slot_tri), n, ptr(tris), ptr(alpha), ptr(shade))
    return tris, alpha, shade


def _patch(w, lib, mats, infos, flags, dirty, tris, alpha, shade):
    lib.resident_patch(C.addressof(w.nodes), NUM_NODES, C.addressof(w.prims), 2, C.addressof(mats), 3, C.addressof(infos), C.addressof(w.textures), 2,
                       ptr(flags), ptr(dirty), len(w.slot_node), ptr(tris), ptr(alpha) if alpha is not None else None,
                       ptr(shade) if shade is not None else None)


MAT_FLAGS = [FORCE_OPAQUE, 0, CULL_DISABLE]  # of the three materials of World.tables()
NEW_NODE_MAT = [1, 1, 0, 2, -3]              # nodes 0, 2, 3, 4 take another material (node 4 a negative id: the record holds max(0, id))


def _set_materials(w, ids):
    for n in range(NUM_NODES):
        w.nodes[n].materialID = ids[n]
    w.node_mat = [max(0, i) for i in ids]


def test_shade_patch_writes_the_material_a_build_writes(lib):
    w = World(5)
    mats, infos = w.tables()
    old_ids = list(w.node_mat)
    tris, alpha, shade = _build(w, lib, mats, infos, _inst_flags(w, MAT_FLAGS))
    assert (shade[:, 5] == np.array(old_ids)[w.slot_node]).all()
    _set_materials(w, NEW_NODE_MAT)
    new_f = _inst_flags(w, MAT_FLAGS)
    want_tris, want_alpha, want_shade = _build(w, lib, mats, infos, new_f)
    assert shade.tobytes() != want_shade.tobytes() and tris.tobytes() != want_tris.tobytes() and alpha.tobytes() != want_alpha.tobytes()
    dirty = np.array([PATCH_SHADE | PATCH_FLAGS | PATCH_ALPHA if NEW_NODE_MAT[n] != old_ids[n] else 0 for n in range(NUM_NODES)], np.uint8)
    _patch(w, lib, mats, infos, new_f, dirty, tris, alpha, shade)
    assert shade.tobytes() == want_shade.tobytes()
    assert tris.tobytes() == want_tris.tobytes()
    assert alpha.tobytes() == want_alpha.tobytes()
    assert (shade[w.slot_node == 4][:, 5] == 0).all()


def test_each_bit_touches_its_own_record_only_and_null_arrays_are_ignored(lib):
    w = World(6)
    mats, infos = w.tables()
    old_f = _inst_flags(w, MAT_FLAGS)
    old = _build(w, lib, mats, infos, old_f)
    _set_materials(w, NEW_NODE_MAT)
    new_f = _inst_flags(w, MAT_FLAGS)
    new = _build(w, lib, mats, infos, new_f)
    for bits in range(8):
        for node in (0, 1, 3):
            tris, alpha, shade = (a.copy() for a in old)
            dirty = np.zeros(NUM_NODES, np.uint8)
            dirty[node] = bits
            _patch(w, lib, mats, infos, new_f, dirty, tris, alpha, shade)
            mine = w.slot_node == node
            for got, was, now, bit in ((tris, old[0], new[0], PATCH_FLAGS), (alpha, old[1], new[1], PATCH_ALPHA), (shade, old[2], new[2], PATCH_SHADE)):
                assert (got[~mine] == was[~mine]).all(), (bits, node)
                assert (got[mine] == (now if bits & bit else was)[mine]).all(), (bits, node, bit)
            # everything of the shade record but the material id stays
            assert (np.delete(shade, 5, axis=1) == np.delete(old[2], 5, axis=1)).all()
    # the caller without shade records (mi_pt_update_materials' bit is never set; a set bit writes nothing)
    tris, alpha, shade = (a.copy() for a in old)
    _patch(w, lib, mats, infos, new_f, np.full(NUM_NODES, 7, np.uint8), tris, None, None)
    assert tris.tobytes() == new[0].tobytes()
