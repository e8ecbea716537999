"""Resident mode (mi_pt_set_accel_resident) and run-time material variants (mi_scene_set_variant) on the GPU: with refits allowed, hidden
render nodes stay in the 8-wide tree, so that a visibility change is a refit and a material-id change a patch of the per-triangle records
instead of a build.  The image does not depend on the tree, so after every step the accumulator, the selection image and the depth image
must equal, bit for bit, what a fresh instance created from the scene's current tables -- visibility array included -- renders.  Also: the
counters of the two info calls, the interplay with the update mode, the fallbacks that still build, queued frames and the headless app."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deform_util as du
import parity_util as pu
from test_gpu_refit import _images, _matrix, _nodes, _render, _rot, _same_as_fresh, _set_matrix, _tracer
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(capi.LIB_DIR, "mi_gltf_renderer")
W, H = 128, 96
REFIT, BUILD = capi.MI_PT_ACCEL_LAST_REFIT, capi.MI_PT_ACCEL_LAST_BUILD


@pytest.fixture(scope="module")
def animated(tmp_path_factory):
    return scenegen.scene_animated(str(tmp_path_factory.mktemp("gpu_resident") / "animated.glb"))


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    return scenegen.scene_variants(str(tmp_path_factory.mktemp("gpu_resident") / "variants.glb"))


def _tri_counts(scene):
    d = scene.desc.contents
    return [int(d.renderPrimitives[d.renderNodes[i].renderPrimID].triangleCount) if d.renderNodes[i].renderPrimID >= 0 else 0 for i in range(d.numRenderNodes)]


def _resident(st, **kw):
    tr = _tracer(st, **kw)
    tr.set_accel_update("refit")
    tr.set_accel_resident(True)
    return tr


def _set_visible(st, tr, hidden):
    """Writes the visibility into the scene's own table (the one a fresh instance is created from) and hands the tables to `tr`."""
    d = st.scene.desc.contents
    for i in range(d.numRenderNodes):
        d.renderNodeVisible[i] = 0 if i in hidden else 1
    tr.update_render_nodes(d.renderNodes, d.numRenderNodes, d.renderNodeVisible)


def _expect_refit(tr, builds, hidden_tris, what):
    a, r = tr.accel_info(), tr.accel_resident_info()
    assert a["builds"] == builds and a["lastUpdate"] == REFIT, (what, a)
    assert r["enabled"] == 1 and r["inForce"] == 1 and r["hiddenTriangles"] == hidden_tris, (what, r)
    return a, r


def test_hide_and_show_refit_like_fresh_instances(animated):
    st = pu.Setup(animated, W, H, max_depth=3)
    n, counts = _nodes(st.scene)[1], _tri_counts(st.scene)
    tr = _resident(st, collect_counters=True)
    a, r = _expect_refit_after_enable(tr, 3)
    assert r["residentTriangles"] >= sum(counts) and r["hiddenTriangles"] == 0 and r["visibilityRefits"] == 0
    want = []
    for _ in range(2):  # (the tree as built, rendered twice: what two renders of one tree differ by)
        tr.reset_stats()
        _render(tr, st)
        want.append(tr.stats())
    steps = [("hide the last", {n - 1}), ("show it", set()), ("hide two", {0, n - 2}), ("hide all", set(range(n))), ("show all", set())]
    for k, (what, hidden) in enumerate(steps):
        _set_visible(st, tr, hidden)
        a, r = _expect_refit(tr, 3, sum(counts[i] for i in hidden), what)
        assert a["refits"] == k + 1 and r["visibilityRefits"] == k + 1 and r["materialPatches"] == 0, (what, a, r)
        assert a["trianglesMoved"] == sum(counts[i] for i in _shown(steps, k)), (what, a)  # what came back; hidden nodes move nothing
        _same_as_fresh(tr, st, what=what)
    a = tr.accel_info()
    assert a["sahCost"] == a["sahCostAtBuild"], a  # back to the all-visible tree, bit for bit
    for _ in range(2):
        tr.reset_stats()
        _render(tr, st)
        got = tr.stats()
        for k in ("nodesClosest", "trisClosest", "nodesShadow", "trisShadow", "nodesPrimary", "trisPrimary"):
            spread = max(abs(want[1][k] - want[0][k]), 1e-2 * want[0][k])  # (the spread of test_no_drift_back_to_the_built_pose)
            assert abs(got[k] - want[0][k]) <= spread, (k, got[k], want[0][k], want[1][k])
    tr.close()


def _shown(steps, k):
    """The render nodes step k brings back: hidden after step k - 1, visible after step k."""
    before = steps[k - 1][1] if k > 0 else set()
    return before - steps[k][1]


def _expect_refit_after_enable(tr, builds):
    a, r = tr.accel_info(), tr.accel_resident_info()
    assert a["builds"] == builds and a["lastUpdate"] == BUILD and a["refitBytes"] > 0, a
    assert r["enabled"] == 1 and r["inForce"] == 1, r
    return a, r


def test_node_hidden_at_creation(animated):
    st = pu.Setup(animated, W, H, max_depth=3)
    n, counts = _nodes(st.scene)[1], _tri_counts(st.scene)
    d = st.scene.desc.contents
    d.renderNodeVisible[n - 1] = 0
    tr = _tracer(st)
    visible_slots = tr.stats()["bvhTriangleCount"]
    tr.set_accel_update("refit")
    tr.set_accel_resident(True)
    a, r = _expect_refit_after_enable(tr, 3)
    assert r["hiddenTriangles"] == counts[n - 1] and r["residentTriangles"] == tr.stats()["bvhTriangleCount"] >= visible_slots + counts[n - 1], r
    assert a["sahCost"] != a["sahCostAtBuild"]  # (the cost at the build is the all-visible one)
    _same_as_fresh(tr, st, what="hidden at creation")
    _set_visible(st, tr, set())
    a, _ = _expect_refit(tr, 3, 0, "shown")
    assert a["sahCost"] == a["sahCostAtBuild"]
    _same_as_fresh(tr, st, what="shown")
    tr.close()


def test_hide_and_move_in_one_update_and_show_what_moved_while_hidden(animated):
    st = pu.Setup(animated, W, H, max_depth=3)
    nodes, n = _nodes(st.scene)
    counts = _tri_counts(st.scene)
    M0 = [_matrix(nodes[i]) for i in range(n)]
    tr = _resident(st)
    # one update: node 1 moves, the last node is hidden
    _set_matrix(nodes[1], _rot(1, 0.4, (0.2, 0.3, 0.0)) @ M0[1])
    _set_visible(st, tr, {n - 1})
    a, _ = _expect_refit(tr, 3, counts[n - 1], "hide + move")
    assert a["trianglesMoved"] == counts[1]
    _same_as_fresh(tr, st, what="hide + move")
    # the hidden node moves: nothing to refit for it
    _set_matrix(nodes[n - 1], _rot(2, 0.5, (0.0, 0.6, 0.3)) @ M0[n - 1])
    _set_visible(st, tr, {n - 1})
    a, _ = _expect_refit(tr, 3, counts[n - 1], "moved while hidden")
    assert a["trianglesMoved"] == 0
    _same_as_fresh(tr, st, what="moved while hidden")
    # ... and comes back where it is now
    _set_visible(st, tr, set())
    a, _ = _expect_refit(tr, 3, 0, "shown at the new matrix")
    assert a["trianglesMoved"] == counts[n - 1]
    _same_as_fresh(tr, st, what="shown at the new matrix")
    tr.close()


def test_hide_and_show_the_largest_atrium_instance(tmp_path):
    """The sliver atrium of test_gpu_refit.py's pre-split case.  (At this detail its resident tree holds one slot per triangle; the case that
    is certain to hold pre-split references is the hall below.)"""
    st = pu.Setup(scenegen.scene_atrium_class(str(tmp_path / "atrium_sliver.glb"), detail=0.25, tex_size=64, sliver=True), W, H, max_depth=2)
    counts = _tri_counts(st.scene)
    big = int(np.argmax(counts))
    tr = _resident(st)
    _set_visible(st, tr, {big})
    _expect_refit(tr, 3, counts[big], "hidden")
    _same_as_fresh(tr, st, what="sliver atrium, largest instance hidden")
    _set_visible(st, tr, set())
    a, _ = _expect_refit(tr, 3, 0, "shown")
    assert a["sahCost"] == a["sahCostAtBuild"]
    _same_as_fresh(tr, st, what="sliver atrium, shown again")
    tr.close()


def test_hide_and_show_pre_split_references(tmp_path):
    """The hall of test_gpu_material_update.py: a two-triangle floor under small spheres, whose triangles the builder pre-splits -- several
    slots per triangle, each filed under a clipped box.  Hidden, every reference is hidden; shown at the build's pose, each gets the clipped
    box it was built with back (the cost is the build's bit for bit); shown after a move, its whole triangle's box."""
    from test_gpu_material_update import _hall
    st = pu.Setup(_hall(str(tmp_path / "hall.glb")), W, H, max_depth=3)
    nodes, n = _nodes(st.scene)
    counts = _tri_counts(st.scene)
    floor = 0
    tr = _resident(st)
    assert tr.stats()["bvhTriangleCount"] > sum(counts)  # splitting engaged: more triangle slots than triangles
    _set_visible(st, tr, {floor})
    _expect_refit(tr, 3, counts[floor], "floor hidden")
    _same_as_fresh(tr, st, what="hall, pre-split floor hidden")
    _set_visible(st, tr, set())
    a, _ = _expect_refit(tr, 3, 0, "floor shown")
    assert a["sahCost"] == a["sahCostAtBuild"]
    _same_as_fresh(tr, st, what="hall, floor shown again")
    _set_visible(st, tr, {floor})
    _set_matrix(nodes[floor], _rot(1, 0.2, (0.0, -0.05, 0.0)) @ _matrix(nodes[floor]))
    _set_visible(st, tr, set())
    _expect_refit(tr, 3, 0, "floor shown after a move")
    _same_as_fresh(tr, st, what="hall, floor moved while hidden, then shown")
    tr.close()


def test_every_node_of_mixed_alpha_glass_hidden_in_turn(tmp_path):
    st = pu.Setup(scenegen.scene_mixed_alpha_glass(str(tmp_path / "mixed.glb")), W, H, max_depth=4)
    n, counts = _nodes(st.scene)[1], _tri_counts(st.scene)
    tr = _resident(st)
    for i in range(n):
        _set_visible(st, tr, {i})
        _expect_refit(tr, 3, counts[i], i)
        _same_as_fresh(tr, st, what="node %d hidden" % i)
    _set_visible(st, tr, set())
    a, _ = _expect_refit(tr, 3, 0, "all shown")
    assert a["sahCost"] == a["sahCostAtBuild"]
    _same_as_fresh(tr, st, what="all shown")
    tr.close()


def test_visibility_clip_plays_without_a_build(tmp_path):
    """scene_material_animated's clip: a KHR_node_visibility blinker (a rebuild per toggle outside resident mode) next to material, light and
    camera channels, at its four key times through update_from_scene."""
    st = pu.Setup(scenegen.scene_material_animated(str(tmp_path / "stage.glb")), W, H, max_depth=4)
    blinker = scenegen.scene_material_animated.LAYOUT["node_blinker"]
    counts = _tri_counts(st.scene)
    tr = _resident(st)
    toggles = 0
    was = 1
    for time in (0.0, 0.6, 1.2, 2.0):
        assert st.scene.update_animation(0, time)
        tr.update_from_scene(st.scene)
        now = int(st.scene.desc.contents.renderNodeVisible[blinker])
        toggles += now != was
        was = now
        _expect_refit(tr, 3, 0 if now else counts[blinker], time)
        cam = st.scene.camera(0)
        st.frame_info = ptmod.camera_frame_info(cam, W, H)[0]
        tr.set_frame_info(st.frame_info)
        _same_as_fresh(tr, st, what=time)
    assert toggles == 2 and tr.accel_resident_info()["visibilityRefits"] == 2
    tr.close()


def test_hidden_skinned_node_comes_back_at_the_current_pose(tmp_path):
    st = pu.Setup(scenegen.scene_skinned(str(tmp_path / "skinned.glb")), W, H, max_depth=3)
    d = st.scene.deformation
    skinned_prims = {p.renderPrimID for p in du.prims(d)}
    desc = st.scene.desc.contents
    hidden = {i for i in range(desc.numRenderNodes) if desc.renderNodes[i].renderPrimID in skinned_prims}
    assert hidden
    counts = _tri_counts(st.scene)
    tr = _tracer(st)
    tr.set_deformation(st.scene)
    tr.set_accel_update("refit")
    tr.set_accel_resident(True)

    def fresh_compare(what):
        streams = {p.renderPrimID: tr.read_vertices(p.renderPrimID) for p in du.prims(d)}
        holder, keep = du.posed_desc(st.scene, streams)
        return _same_as_fresh(tr, st, holder, what)
    rest = fresh_compare("rest")
    _set_visible(st, tr, hidden)
    _expect_refit(tr, 3, sum(counts[i] for i in hidden), "hidden")
    fresh_compare("hidden")
    assert st.scene.update_animation(0, 1.4)
    tr.update_from_scene(st.scene)  # (deforms, then hands over the tables: the node stays hidden)
    a, _ = _expect_refit(tr, 3, sum(counts[i] for i in hidden), "hidden, clip advanced")
    fresh_compare("hidden, clip advanced")
    _set_visible(st, tr, set())
    _expect_refit(tr, 3, 0, "shown")
    posed = fresh_compare("shown at the current pose")
    assert not (posed == rest).all()
    tr.close()


def _switch(st, tr, v):
    changed = st.scene.set_variant(v)
    d = st.scene.desc.contents
    tr.update_render_nodes(d.renderNodes, d.numRenderNodes, d.renderNodeVisible)
    return changed


def test_variant_cycle_patches_like_fresh_instances(variants):
    st = pu.Setup(variants, W, H, max_depth=4)
    counts = _tri_counts(st.scene)
    tr = _resident(st)
    split_refs = tr.stats()["bvhTriangleCount"] > sum(counts)
    builds, patches = 3, 0
    # OPAQUE -> MASK: the alpha records appear; MASK -> glass: they stay (a transmissive instance is not opaque); glass -> base: they go
    for v, records in ((1, +1), (2, 0), (0, -1)):
        slots, last_bytes = tr.stats()["bvhTriangleCount"], tr.memory()["sceneBytes"]
        assert _switch(st, tr, v) > 0
        transmissive_flip = v in (2, 0)  # sphere B takes, then leaves, the transmissive material
        a, r = tr.accel_info(), tr.accel_resident_info()
        if transmissive_flip and split_refs:
            builds += 1
            assert a["lastUpdate"] == BUILD, (v, a)
        else:
            patches += 1
            assert a["lastUpdate"] == REFIT, (v, a)
        assert a["builds"] == builds and r["materialPatches"] == patches and r["inForce"] == 1, (v, a, r)
        if a["lastUpdate"] == REFIT:
            now = tr.memory()["sceneBytes"]
            assert now - last_bytes == records * 48 * slots, (v, now, last_bytes)
        _same_as_fresh(tr, st, what="variant %d" % v)
    assert a["refits"] == 0  # a material switch alone sweeps no level
    # a switch, a move and a hidden node in ONE update
    nodes, n = _nodes(st.scene)
    _set_matrix(nodes[3], _rot(1, 0.3, (0.1, 0.2, 0.0)) @ _matrix(nodes[3]))
    st.scene.set_variant(1)
    _set_visible(st, tr, {n - 1})
    a, r = _expect_refit(tr, builds, counts[n - 1], "switch + move + hide")
    assert r["materialPatches"] == patches + 1 and r["visibilityRefits"] == 1 and a["refits"] == 1
    _same_as_fresh(tr, st, what="switch + move + hide")
    # the material of a HIDDEN node switches: it comes back with the new one
    st.scene.set_variant(0)
    _set_visible(st, tr, {n - 1})
    _set_visible(st, tr, set())
    _same_as_fresh(tr, st, what="hidden node switched, then shown")
    assert tr.accel_info()["builds"] == builds
    tr.close()


def test_variant_switch_with_resident_mode_off_rebuilds(variants):
    """Today's behaviour, pinned: under REFIT without resident mode a material-id change is a build."""
    st = pu.Setup(variants, W, H, max_depth=4)
    tr = _tracer(st)
    tr.set_accel_update("refit")
    for k, v in enumerate((1, 2, 0)):
        assert _switch(st, tr, v) > 0
        a, r = tr.accel_info(), tr.accel_resident_info()
        assert a["lastUpdate"] == BUILD and a["builds"] == 3 + k and a["refits"] == 0, a
        assert r == {"enabled": 0, "inForce": 0, "residentTriangles": 0, "hiddenTriangles": 0, "visibilityRefits": 0, "materialPatches": 0}, r
        _same_as_fresh(tr, st, what="variant %d, resident mode off" % v)
    tr.close()


def test_alpha_change_on_cut_geometry_is_refused_with_nothing_changed(variants):
    st = pu.Setup(variants, W, H, max_depth=3)
    st.scene.set_variant(1)
    st.scene.cut_alpha(4)
    tr = _resident(st)
    before = _images(tr, st)
    d = st.scene.desc.contents
    table = (capi.MiGltfRenderNode * d.numRenderNodes)()
    C.memmove(table, d.renderNodes, C.sizeof(table))
    table[1].materialID = scenegen.scene_variants.LAYOUT["red"]  # the cut sphere: MASK -> OPAQUE
    with pytest.raises(ptmod.MiError) as e:
        tr.update_render_nodes(table, d.numRenderNodes, d.renderNodeVisible)
    assert "cut at load" in str(e.value)
    a, r = tr.accel_info(), tr.accel_resident_info()
    assert a["builds"] == 3 and r["materialPatches"] == 0
    after = _images(tr, st)
    assert all((x == y).all() for x, y in zip(before, after))
    tr.close()


def test_mode_interplay(animated, monkeypatch):
    st = pu.Setup(animated, W, H, max_depth=2)
    nodes, n = _nodes(st.scene)
    counts = _tri_counts(st.scene)
    st.scene.desc.contents.renderNodeVisible[n - 1] = 0
    vis = st.scene.desc.contents.renderNodeVisible
    # enabling under REBUILD is inert until the mode allows refits; either order of the two calls ends in the same state
    a_ = _tracer(st)
    visible_slots = a_.stats()["bvhTriangleCount"]
    a_.set_accel_resident(True)
    assert a_.accel_info()["builds"] == 1 and a_.accel_resident_info() == {"enabled": 1, "inForce": 0, "residentTriangles": 0, "hiddenTriangles": 0,
                                                                          "visibilityRefits": 0, "materialPatches": 0}
    a_.update_render_nodes(nodes, n, vis)  # (inert: an update under REBUILD builds, over the visible nodes)
    assert a_.accel_info()["builds"] == 2 and a_.stats()["bvhTriangleCount"] == visible_slots
    a_.set_accel_update("refit")
    b_ = _tracer(st)
    b_.set_accel_update("refit")
    b_.set_accel_resident(True)
    ia, ib = a_.accel_resident_info(), b_.accel_resident_info()
    assert ia == ib and ia["inForce"] == 1 and ia["hiddenTriangles"] == counts[n - 1], (ia, ib)
    assert a_.accel_info()["builds"] == 3 and b_.accel_info()["builds"] == 3
    for k in ("sahCost", "sahCostAtBuild", "refitBytes", "mode"):
        assert a_.accel_info()[k] == b_.accel_info()[k], k
    assert a_.stats()["bvhTriangleCount"] == b_.stats()["bvhTriangleCount"] == visible_slots + counts[n - 1]
    assert a_.memory()["sceneBytes"] == b_.memory()["sceneBytes"]
    a_.close()
    # disabling rebuilds over the visible nodes only; enabling again is a build too
    b_.set_accel_resident(False)
    assert b_.accel_info()["builds"] == 4 and b_.stats()["bvhTriangleCount"] == visible_slots
    assert b_.accel_resident_info()["inForce"] == 0 and b_.accel_resident_info()["enabled"] == 0
    b_.set_accel_resident(False)
    assert b_.accel_info()["builds"] == 4
    _same_as_fresh(b_, st, what="disabled")
    # REFIT -> REBUILD drops the refit data: out of force at once, and the next update builds over the visible nodes
    b_.set_accel_resident(True)
    assert b_.accel_info()["builds"] == 5 and b_.accel_resident_info()["inForce"] == 1
    b_.set_accel_update("rebuild")
    assert b_.accel_resident_info()["inForce"] == 0 and b_.accel_resident_info()["enabled"] == 1
    _same_as_fresh(b_, st, what="rebuild mode over the resident tree")
    b_.update_render_nodes(nodes, n, None)
    assert b_.accel_info()["builds"] == 6 and b_.accel_info()["lastUpdate"] == BUILD
    b_.close()
    # the BVH2 walk and the host collapse keep no refit data: resident mode stays inert, their updates build
    c_ = _tracer(st, bvh=1)
    c_.set_accel_update("refit")
    c_.set_accel_resident(True)
    assert c_.accel_info()["builds"] == 1 and c_.accel_resident_info()["inForce"] == 0
    c_.update_render_nodes(nodes, n, None)
    assert c_.accel_info()["lastUpdate"] == BUILD and c_.accel_info()["builds"] == 2
    c_.close()
    monkeypatch.setenv("MI_PT_HOST_COLLAPSE", "1")  # (read once, in mi_pt_create; the host collapse is the greedy one)
    monkeypatch.setenv("MI_PT_COLLAPSE", "greedy")
    d_ = _tracer(st)
    monkeypatch.delenv("MI_PT_HOST_COLLAPSE")
    monkeypatch.delenv("MI_PT_COLLAPSE")
    d_.set_accel_update("refit")
    d_.set_accel_resident(True)
    assert d_.accel_resident_info()["inForce"] == 0 and d_.accel_info()["refitBytes"] == 0
    builds = d_.accel_info()["builds"]
    d_.update_render_nodes(nodes, n, vis)
    assert d_.accel_info()["lastUpdate"] == BUILD and d_.accel_info()["builds"] == builds + 1
    _same_as_fresh(d_, st, what="host collapse")
    d_.close()


def test_queued_frames_render_the_old_state(animated):
    ref_st = pu.Setup(animated, W, H, max_depth=3)
    ref = _tracer(ref_st)
    want = _render(ref, ref_st, 3)
    ref.close()
    st = pu.Setup(animated, W, H, max_depth=3)
    n = _nodes(st.scene)[1]
    q = _resident(st)
    q.set_frame_queue(8)
    total = 0
    for f in range(3):
        p = st.frame_params(f, total)
        q.render_frame(p)
        total += p.numSamples
    _set_visible(st, q, {n - 1})  # flushes the three queued frames first: they render the node
    assert (q.read_accum() == want).all()
    assert q.accel_info()["lastUpdate"] == REFIT
    _same_as_fresh(q, st, what="after the flush")
    q.close()


def test_headless_variant_through_resident_mode_writes_the_same_file(tmp_path, assets, variants):
    hdr = os.path.join(assets, "std_env.hdr")
    common = ["--headless", "--size", "160", "96", "--scenefile", variants, "--hdrfile", hdr, "--ptSamples", "1", "--ptAdaptiveSampling", "0", "--envSystem", "1",
              "--ptMaxDepth", "4", "--frames", "3", "--maxFrames", "100"]
    files = {}
    for name, extra in (("base", []), ("variant", ["--variant", "1"]), ("resident", ["--variant", "1", "--accelUpdate", "1", "--accelResident", "1"])):
        out = tmp_path / (name + ".hdr")
        r = subprocess.run([APP] + common + extra + ["--output", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "variant:" not in r.stderr, r.stdout + r.stderr
        files[name] = out.read_bytes()
    assert files["resident"] == files["variant"]
    assert files["variant"] != files["base"]
