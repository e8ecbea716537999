"""Caller-driven vertices on the device (mi_pt_set_vertex_updates / mi_pt_update_vertices / mi_pt_update_vertices_device;
csrc/device/vertex_update.hip): an updated instance renders bit for bit what a fresh instance of the same vertices renders -- under every
acceleration-update mode and both builders, against the oracle, with partial streams and rebuilt normals, over pre-split references --
the device form equals the host form and rejects non-finite vertices, every refusal leaves the instance untouched, and vertex motion follows
the declared primitives."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import deform_util as du
import parity_util as pu
import temporal_util as tu
import vertex_motion_util as vmu
import vertex_update_util as vu
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES, DEPTH = 128, 96, 2, 3
CLOTH, BALL, BOX, TRIANGLE = 336, 325, 24, 3  # vertex counts of scene_dynamic's dynamic primitives


@pytest.fixture(scope="module")
def dynamic(tmp_path_factory):
    return scenegen.scene_dynamic(str(tmp_path_factory.mktemp("gpu_vertex_update") / "dynamic.glb"))


def _setup(path, **kw):
    return pu.Setup(path, W, H, max_depth=DEPTH, **kw)


def _tracer(st, scene=None, bvh=0):
    tr = ptmod.PathTracer(scene if scene is not None else st.scene, bvh=bvh)
    tr.resize(st.width, st.height)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    return tr


def _render(tr, st, frames=FRAMES):
    total = 0
    for f in range(frames):
        p = st.frame_params(f, total)
        tr.render_frame(p)
        total += p.numSamples
    return tr.read_accum()


def _prim_of(scene):
    """{vertex count: render primitive} of the scene (scene_dynamic's primitives all differ in size)."""
    d = scene.desc.contents
    return {int(d.renderPrimitives[i].vertexCount): i for i in range(int(d.numRenderPrimitives))}


def _rest(scene, pid):
    rp = scene.desc.contents.renderPrimitives[pid]
    nv = int(rp.vertexCount)
    get = lambda ptr, w: du.arr(ptr, nv * w).reshape(nv, w) if ptr else None  # noqa: E731
    return dict(pos=get(rp.positions, 3), nrm=get(rp.normals, 3), tan=get(rp.tangents, 4), uv0=get(rp.texCoords0, 2),
                idx=du.arr(rp.indices, int(rp.triangleCount) * 3, np.uint32).reshape(-1, 3))


def _poses(scene):
    """Three successive updates of the four dynamic primitives: {primitive: (positions, normals or None, tangents or None)}."""
    ids = _prim_of(scene)
    rest = {k: _rest(scene, ids[k]) for k in (CLOTH, BALL, BOX, TRIANGLE)}
    out = []
    for k in range(3):
        out.append({ids[CLOTH]: vu.cloth_wave(rest[CLOTH]["pos"], 0.5 + 1.3 * k),
                    ids[BALL]: vu.ball_pulse(rest[BALL]["pos"], rest[BALL]["nrm"], 0.9 * k) + (None,),
                    ids[BOX]: (vu.box_shear(rest[BOX]["pos"], 0.3 + 0.25 * k), None, None),
                    ids[TRIANGLE]: (vu.triangle_move(rest[TRIANGLE]["pos"], (0.1 * k, 0.05 + 0.1 * k, -0.2 * k)), None, None)})
    return out


def _fresh(st, streams, bvh=0):
    """Accumulator and selection image of a fresh instance created from the scene's tables with `streams` for vertices."""
    holder, keep = du.posed_desc(st.scene, streams)
    fresh = _tracer(st, holder, bvh)
    try:
        return _render(fresh, st), fresh.read_selection()
    finally:
        fresh.close()
        del keep


def _same(a, b):
    return (a is None and b is None) or np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _streams_equal(tr, pid, want):
    got = tr.read_vertices(pid)
    return all(w is None or _same(g, w) for g, w in zip(got, want))


def _rc(call):
    with pytest.raises(ptmod.MiError) as e:
        call()
    return str(e.value)


_fresh_cache = {}


def _fresh_of_pose(st, poses, k, bvh):
    """The fresh-instance images of pose k (what the earlier updates left of the streams a later one does not bring is the rest pose's here:
    every pose brings the same streams).  One instance per pose and builder, shared by the modes."""
    if (k, bvh) not in _fresh_cache:
        _fresh_cache[(k, bvh)] = _fresh(st, poses[k], bvh)
    return _fresh_cache[(k, bvh)]


# ---- 1. fresh-instance identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,bvh", [("rebuild", 0), ("refit", 0), ("auto", 0), ("rebuild", 1)])
def test_updated_instance_renders_what_a_fresh_instance_renders(dynamic, mode, bvh):
    st = _setup(dynamic)
    poses = _poses(st.scene)
    tr = _tracer(st, bvh=bvh)
    try:
        tr.set_accel_update(mode)
        tr.set_vertex_updates(sorted(poses[0]))
        rest = _render(tr, st)
        d = st.scene.desc.contents
        for k, pose in enumerate(poses):
            a = tr.accel_info()
            tr.update_vertices(pose)
            b = tr.accel_info()
            assert b["builds"] + b["refits"] == a["builds"] + a["refits"] + 1, (k, a, b)
            if mode == "refit" and bvh == 0:
                assert b["refits"] == a["refits"] + 1 and b["lastUpdate"] == capi.MI_PT_ACCEL_LAST_REFIT
            if mode == "rebuild":
                assert b["builds"] == a["builds"] + 1 and b["refits"] == 0
            for pid, streams in pose.items():
                assert _streams_equal(tr, pid, streams), (k, pid)
            img, sel = _render(tr, st), tr.read_selection()
            want, want_sel = _fresh_of_pose(st, poses, k, bvh)
            assert (img == want).all(), (mode, bvh, k, float(np.abs(img - want).max()))
            assert (sel == want_sel).all(), (mode, bvh, k)
            assert not (img == rest).all() and np.isfinite(img).all()
        info = tr.vertex_update_info()
        assert info["calls"] == 3 and info["verticesWritten"] == 3 * (CLOTH + BALL + BOX + TRIANGLE) and info["verticesRejected"] == 0
        # a deferred build: nothing until the node update that follows, then one build or refit for both
        a = tr.accel_info()
        tr.update_vertices(poses[0], defer_build=True)
        b = tr.accel_info()
        assert (b["builds"], b["refits"]) == (a["builds"], a["refits"])
        tr.update_render_nodes(d.renderNodes, d.numRenderNodes, d.renderNodeVisible)
        c = tr.accel_info()
        assert c["builds"] + c["refits"] == a["builds"] + a["refits"] + 1
        want, want_sel = _fresh_of_pose(st, poses, 0, bvh)
        assert (_render(tr, st) == want).all() and (tr.read_selection() == want_sel).all()
    finally:
        tr.close()


# ---- 2. the oracle ----------------------------------------------------------------------------------------------------------------------
def test_updated_pose_against_the_oracle(dynamic):
    st = _setup(dynamic)
    pose = _poses(st.scene)[1]
    tr = _tracer(st)
    try:
        tr.set_vertex_updates(sorted(pose))
        tr.update_vertices(pose)
        img, sel = _render(tr, st), tr.read_selection()
    finally:
        tr.close()
    holder, keep = du.posed_desc(st.scene, pose)
    posed = copy.copy(st)
    posed.scene = holder
    ref = pu.render_oracle(posed, FRAMES)
    cmp = pu.compare_images(ref["accum"], img)
    agree = float((ref["selection"] == sel).mean())
    print("updated pose vs oracle", cmp, "selection agreement", agree)
    assert cmp["rel_l2"] < 5e-3 and agree >= 0.999, (cmp, agree)
    del keep


# ---- 3. partial streams -----------------------------------------------------------------------------------------------------------------
def test_partial_streams_and_rebuilt_normals(dynamic):
    st = _setup(dynamic)
    cloth = _prim_of(st.scene)[CLOTH]
    rest = _rest(st.scene, cloth)
    pos = vu.cloth_wave(rest["pos"], 0.8)[0]
    # positions only: normals, tangents and uv0 keep their bytes
    tr = _tracer(st)
    try:
        tr.set_vertex_updates([cloth])
        assert tr.vertex_update_info()["tableBytes"] == 0
        tr.update_vertices({cloth: pos})
        gp, gn, gt = tr.read_vertices(cloth)
        assert _same(gp, pos) and _same(gn, rest["nrm"]) and _same(gt, rest["tan"])
        img, sel = _render(tr, st), tr.read_selection()
        want, want_sel = _fresh(st, {cloth: (pos, None, None)})  # (uv0: a fresh instance takes the file's, so the image says it stayed)
        assert (img == want).all() and (sel == want_sel).all()
    finally:
        tr.close()
    # positions only with RECOMPUTE_NORMALS: the float64 definition within 2e-6, tangents unchanged, the image a fresh instance's
    tr = _tracer(st)
    try:
        tr.set_vertex_updates([cloth], recompute_normals=True)
        assert tr.vertex_update_info()["tableBytes"] == 4 * rest["idx"].size + 4 * CLOTH
        tr.update_vertices({cloth: pos})
        gp, gn, gt = tr.read_vertices(cloth)
        want_n, kept = vu.rebuilt_normals_f64(pos, rest["idx"], rest["nrm"])
        err = float(np.abs(gn - want_n).max())
        print("rebuilt normals: max |n - n64| = %.3g (bound %.3g)" % (err, vu.NORMAL_BOUND))
        assert _same(gp, pos) and _same(gt, rest["tan"]) and not kept.any()
        assert err <= vu.NORMAL_BOUND, err
        assert np.abs(gn - rest["nrm"]).max() > 0.1  # (they did change)
        img, sel = _render(tr, st), tr.read_selection()
        want, want_sel = _fresh(st, {cloth: (gp, gn, gt)})
        assert (img == want).all() and (sel == want_sel).all()
        # supplied normals win over the rebuild
        given = vu.cloth_wave(rest["pos"], 0.8)[1]
        tr.update_vertices({cloth: (pos, given, None)})
        assert _same(tr.read_vertices(cloth)[1], given)
    finally:
        tr.close()


# ---- 4. pre-split references ------------------------------------------------------------------------------------------------------------
def test_scaled_pre_split_primitive_under_refit(tmp_path):
    path = scenegen.scene_atrium_class(str(tmp_path / "atrium_sliver.glb"), detail=0.25, tex_size=64, sliver=True)
    st = pu.Setup(path, W, H, max_depth=2)
    d = st.scene.desc.contents
    nodes, n = d.renderNodes, int(d.numRenderNodes)
    counts = [int(d.renderPrimitives[nodes[i].renderPrimID].triangleCount) if nodes[i].renderPrimID >= 0 else 0 for i in range(n)]
    big = int(nodes[int(np.argmax(counts))].renderPrimID)  # the primitive tests/test_gpu_refit.py::test_moved_pre_split_instance moves
    tr = _tracer(st)
    try:
        tr.set_accel_update("refit")
        tr.set_vertex_updates([big])
        rest = _render(tr, st)
        for k in range(2):
            pos, nrm, tan = tr.read_vertices(big)
            pos = (pos * np.float32(1.02)).astype(np.float32)
            before = tr.accel_info()
            tr.update_vertices({big: pos})
            after = tr.accel_info()
            assert after["refits"] == before["refits"] + 1 and after["builds"] == before["builds"], (k, before, after)
            img, sel = _render(tr, st), tr.read_selection()
            want, want_sel = _fresh(st, {big: (pos, nrm, tan)})
            assert (img == want).all() and (sel == want_sel).all(), k
            assert not (img == rest).all()
    finally:
        tr.close()


# ---- 5. the device form -----------------------------------------------------------------------------------------------------------------
def test_device_form_with_torch_tensors(tmp_path):
    """In a process of its own (tests/vertex_update_device_child.py): torch brings its own copy of the HIP runtime, and the two libraries share
    one only when torch is loaded first.  The child checks that torch tensors go in and the read-back streams and the image equal the host
    form's bit for bit, that the call allocates nothing, and that a tensor with 5 non-finite vertices among 336 leaves exactly those at their
    resident bytes, reports 5 rejected, and is followed by a finite refit and render."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vertex_update_device_child.py"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "VERTEX_UPDATE_DEVICE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---- 6. arguments and state -------------------------------------------------------------------------------------------------------------
def _raw(tr, entries, flags=0, device=False):
    """mi_pt_update_vertices with a hand-made table: entries = [(prim, vertexCount, positions, normals, tangents, reserved)]."""
    table = (capi.MiPtVertexUpdate * max(len(entries), 1))()
    for u, (prim, nv, p, n, t, reserved) in zip(table, entries):
        u.renderPrimID, u.vertexCount = prim, nv
        u.positions, u.normals, u.tangents = (None if a is None else a.ctypes.data for a in (p, n, t))
        u.reserved[0], u.reserved[1] = reserved
    fn = tr._l.mi_pt_update_vertices_device if device else tr._l.mi_pt_update_vertices
    return fn(tr._p, table, len(entries), flags)


def test_refusals_leave_the_instance_untouched(dynamic):
    st = _setup(dynamic)
    ids = _prim_of(st.scene)
    cloth, ball, box, tri = ids[CLOTH], ids[BALL], ids[BOX], ids[TRIANGLE]
    pose = _poses(st.scene)[0]
    num_prims = int(st.scene.desc.contents.numRenderPrimitives)
    tr = _tracer(st)
    try:
        tr.set_accel_update("refit")
        bare = tr.memory()
        assert tr.vertex_update_info() == dict(calls=0, verticesWritten=0, verticesRejected=0, tableBytes=0)
        assert _raw(tr, [(cloth, CLOTH, pose[cloth][0], None, None, (0, 0))]) == -4  # MI_PT_ERR_STATE: nothing declared
        # the declaration's own refusals: nothing declared afterwards
        for bad in ([cloth, num_prims], [-1], [cloth, ball, cloth]):
            assert "rc=-1" in _rc(lambda: tr.set_vertex_updates(bad))
        arr = (C.c_int32 * 1)(cloth)
        assert tr._l.mi_pt_set_vertex_updates(tr._p, arr, 1, 2) == -1  # an unknown flag bit
        assert _raw(tr, [(cloth, CLOTH, pose[cloth][0], None, None, (0, 0))]) == -4
        assert tr.memory()["sceneBytes"] == bare["sceneBytes"] and tr.memory()["rendererBytes"] == bare["rendererBytes"]
        tr.set_vertex_updates([cloth, ball, tri], recompute_normals=True)  # (the box stays undeclared)
        table = tr.vertex_update_info()["tableBytes"]
        assert table == 4 * (3 * 600 + CLOTH) + 4 * (3 * 576 + BALL)  # (the triangle has no normal stream: no table)
        declared = tr.memory()
        assert declared["sceneBytes"] >= bare["sceneBytes"] + table and declared["rendererBytes"] == bare["rendererBytes"]
        tr.update_vertices({cloth: pose[cloth], ball: pose[ball]})  # (the staging buffer exists from here on)
        state = lambda: (tr.memory()["sceneBytes"], tr.memory()["rendererBytes"], tr.accel_info(), tr.vertex_update_info(),  # noqa: E731
                         [a.tobytes() for p in (cloth, ball, box, tri) for a in tr.read_vertices(p) if a is not None])
        before = state()
        assert before[1] > declared["rendererBytes"]
        cp, cn, ct = pose[cloth]
        tp = pose[tri][0]
        nan_p, inf_n, inf_t = cp.copy(), cn.copy(), ct.copy()
        nan_p[335, 2], inf_n[0, 0], inf_t[100, 3] = np.nan, np.inf, -np.inf
        ok = (cloth, CLOTH, vu.cloth_wave(cp, 2.0)[0], None, None, (0, 0))
        refused = {
            "undeclared": [ok, (box, BOX, pose[box][0], None, None, (0, 0))],
            "out of range": [ok, (num_prims, 3, tp, None, None, (0, 0))],
            "repeated": [ok, ok],
            "vertex count": [ok, (ball, BALL - 1, pose[ball][0], None, None, (0, 0))],
            "null positions": [ok, (ball, BALL, None, None, None, (0, 0))],
            "normals for no stream": [ok, (tri, TRIANGLE, tp, tp, None, (0, 0))],
            "tangents for no stream": [ok, (ball, BALL, pose[ball][0], None, np.zeros((BALL, 4), np.float32), (0, 0))],
            "reserved 0": [ok, (tri, TRIANGLE, tp, None, None, (1, 0))],
            "reserved 1": [ok, (tri, TRIANGLE, tp, None, None, (0, 7))],
            "nan position": [(tri, TRIANGLE, tp, None, None, (0, 0)), (cloth, CLOTH, nan_p, cn, ct, (0, 0))],
            "inf normal": [(tri, TRIANGLE, tp, None, None, (0, 0)), (cloth, CLOTH, cp, inf_n, ct, (0, 0))],
            "inf tangent": [(tri, TRIANGLE, tp, None, None, (0, 0)), (cloth, CLOTH, cp, cn, inf_t, (0, 0))],
        }
        for why, entries in refused.items():
            assert _raw(tr, entries) == -1, why
            assert state() == before, why
        assert _raw(tr, [ok], flags=2) == -1 and _raw(tr, [ok], flags=2, device=True) == -1 and state() == before  # unknown flag bits
        # the frame queue is flushed: frames recorded before an update show the old vertices
        _render(tr, st)
        old = tr.read_accum()
        tr.set_frame_queue(4)
        total = 0
        for f in range(2):
            p = st.frame_params(f, total)
            tr.render_frame(p)  # (held back)
            total += p.numSamples
        tr.update_vertices({cloth: vu.cloth_wave(cp, 2.0)})
        assert (tr.read_accum() == old).all()
        tr.set_frame_queue(1)
        assert not (_render(tr, st) == old).all()
        # releasing the declaration frees the tables; the staging buffer stays with the renderer
        staged = tr.memory()["rendererBytes"]
        for release in (lambda: tr.set_vertex_updates(None), lambda: tr.set_vertex_updates([])):
            tr.set_vertex_updates([cloth], recompute_normals=True)
            release()
            m = tr.memory()
            assert tr.vertex_update_info()["tableBytes"] == 0 and m["rendererBytes"] == staged
            assert _raw(tr, [ok]) == -4
    finally:
        tr.close()
    # an instance that never declares anything holds what one that declared and released holds, and what it held before the feature:
    # no table, no task array, no staging
    a, b = _tracer(st), _tracer(st)
    try:
        a.set_accel_update("refit")  # (as `bare` was measured: the refit data is part of sceneBytes)
        b.set_accel_update("refit")
        b.set_vertex_updates([cloth, ball], recompute_normals=True)
        b.set_vertex_updates(None)
        ma, mb = a.memory(), b.memory()
        assert all(ma[k] == mb[k] for k in ("sceneBytes", "rendererBytes", "pathStateBytes", "pathSlots")), (ma, mb)
        assert ma["sceneBytes"] == bare["sceneBytes"] and ma["rendererBytes"] == bare["rendererBytes"]
        assert a.vertex_update_info() == dict(calls=0, verticesWritten=0, verticesRejected=0, tableBytes=0)
        assert (_render(a, st) == _render(b, st)).all()
    finally:
        a.close()
        b.close()


def test_deformation_tables_and_declarations_exclude_each_other(tmp_path):
    st = _setup(scenegen.scene_skinned(str(tmp_path / "skinned.glb")))
    deforming = [int(p.renderPrimID) for p in du.prims(st.scene.deformation)]
    static = [p for p in range(int(st.scene.desc.contents.numRenderPrimitives)) if p not in deforming][0]
    tr = _tracer(st)
    try:
        tr.set_deformation(st.scene)
        assert "rc=-1" in _rc(lambda: tr.set_vertex_updates([static, deforming[0]]))
        tr.set_vertex_updates([static])  # a primitive the tables leave alone is fine
        tr.set_deformation(None)
        tr.set_vertex_updates([deforming[0]])
        assert "rc=-1" in _rc(lambda: tr.set_deformation(st.scene))
        tr.set_vertex_updates(None)
        tr.set_deformation(st.scene)
    finally:
        tr.close()


# ---- 7. vertex motion -------------------------------------------------------------------------------------------------------------------
TOL_PX, TOL_Z = 1e-3 * W / 1920.0, 2e-6  # the bounds tests/test_gpu_vertex_motion.py holds the motion image to


def test_vertex_motion_follows_the_declared_primitive(dynamic):
    st = _setup(dynamic)
    ids = _prim_of(st.scene)
    cloth, ball = ids[CLOTH], ids[BALL]
    rest = _rest(st.scene, cloth)
    d = st.scene.desc.contents
    n = int(d.numRenderNodes)
    o2w = np.array([d.renderNodes[i].objectToWorld[:] for i in range(n)], np.float32)
    w2o = np.array([d.renderNodes[i].worldToObject[:] for i in range(n)], np.float32)
    node_prims = np.array([d.renderNodes[i].renderPrimID for i in range(n)], np.int64)
    st.frame_info.prevMVP[:] = st.frame_info.viewProjMatrix[:]  # (the camera stands still)
    vp = np.array(st.frame_info.viewProjMatrix[:], np.float32)
    tr = _tracer(st)
    try:
        tr.set_vertex_motion(True)
        tr.set_temporal(True)
        assert "rc=-4" in _rc(lambda: tr.read_previous_positions(cloth))  # inert: nothing deforms, nothing is declared
        tr.set_vertex_updates([cloth])
        assert _same(tr.read_previous_positions(cloth), rest["pos"])
        assert "rc=-1" in _rc(lambda: tr.read_previous_positions(ball))
        a = vu.cloth_wave(rest["pos"], 0.4)
        # (the wave moves the cloth along the view axis, a fraction of a pixel on screen: slide it sideways too, 0.15 units ~ 3.5 pixels)
        a = ((a[0] + np.array([0.15, 0.0, 0.0], np.float32)).astype(np.float32),) + a[1:]
        tr.update_vertices({cloth: a})
        assert _same(tr.read_previous_positions(cloth), rest["pos"])  # the previous positions follow the RENDERED pose
        first = st.frame_params(0, 0)
        tr.render_frame(first)
        motion, fh, tri = tr.read_motion(), tr.read_first_hit(), tr.read_first_hit_triangle()
        assert _same(tr.read_previous_positions(cloth), a[0])
        prims = {cloth: dict(indices=rest["idx"], cur=a[0], prev=rest["pos"])}
        want, _, took = vmu.vertex_motion_numpy(fh.reshape(-1, 4), tri.reshape(-1, 4), prims, o2w, w2o, o2w, vp, vp, W, H)
        want, took = want.reshape(H, W, 3), took.reshape(H, W)
        hit = np.ascontiguousarray(fh[..., 3]).view(np.uint32).astype(np.int64)
        mesh = (hit != 0) & (hit != tu.ID_INVALID)
        on_cloth = mesh & (np.where(mesh, node_prims[np.clip(hit - 1, 0, n - 1)], -1) == cloth)
        e_xy = float(np.abs(motion[..., :2] - want[..., :2])[on_cloth].max())
        e_z = float(np.abs(motion[..., 2] - want[..., 2])[on_cloth].max())
        print("cloth pixels: %d, on the deformed path %d, |delta| %.3g px (bound %.3g), depth %.3g, largest motion %.2f px" % (
            on_cloth.sum(), took.sum(), e_xy, TOL_PX, e_z, np.abs(want[..., :2])[on_cloth].max()))
        assert on_cloth.mean() >= 0.05 and took.sum() > 0.5 * on_cloth.sum() and not (took & ~on_cloth).any()
        assert e_xy <= TOL_PX and e_z <= TOL_Z
        assert np.abs(want[..., :2])[on_cloth].max() > 1.0
        assert (motion[..., :2][~on_cloth] == 0.0).all()  # camera and nodes stood still
        # a second batch without an update: exactly zero motion
        tr.render_frame(first)
        assert (tr.read_motion()[..., :2] == 0.0).all()
        assert _same(tr.read_previous_positions(cloth), a[0])
        # releasing the declaration makes vertex motion inert again
        tr.set_vertex_updates(None)
        assert "rc=-4" in _rc(lambda: tr.read_previous_positions(cloth))
    finally:
        tr.close()
