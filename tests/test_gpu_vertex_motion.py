"""Vertex motion on the device (mi_pt_set_vertex_motion, mi_pt_read_first_hit_triangle, mi_pt_read_previous_positions; csrc/device/temporal.hip,
pt_temporal.h: motionRecordDeformed): off changes nothing, the triangle record is the first hit, the previous positions follow the rendered
pose, the motion image against the float64 restatement of tests/vertex_motion_util.py fed the read-back inputs, still characters have
exactly zero motion, refit, refusals and memory, the temporal stage on the new motion, and the headless app's --vertexMotion."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deform_util as du
import parity_util as pu
import temporal_util as tu
import vertex_motion_util as vu
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 128, 96
TA, TB = 0.6, 1.4  # the two times of clip "pose" the sequences render
PARAMS = dict(alpha=0.2, momentsAlpha=0.2, maxHistory=32.0, normalCos=0.9, depthTolerance=0.1)
SIGMAS = dict(sigmaLuminance=4.0, sigmaNormal=128.0, sigmaDepth=1.0)
TOL_PX, TOL_Z = 1e-3 * W / 1920.0, 2e-6  # the bounds of test_gpu_temporal.py's motion test


@pytest.fixture(scope="module")
def skinned(tmp_path_factory):
    return scenegen.scene_skinned(str(tmp_path_factory.mktemp("gpu_vertex_motion") / "skinned.glb"))


def _setup(path, w=W, h=H):
    return pu.Setup(path, w, h, max_depth=3, spp_per_frame=1, params_edit=lambda p: setattr(p, "flags", p.flags | capi.MI_PT_USE_OPTIX_DENOISER))


def _tracer(s, vertex_motion=True, temporal=True, deform=True, tile=None):
    tr = ptmod.PathTracer(s.scene)
    if tile is not None:
        tr.set_tile_partition(*tile)
    tr.resize(s.width, s.height)
    s.frame_info.prevMVP[:] = s.frame_info.viewProjMatrix[:]  # (a camera that stands still, until a test says otherwise)
    tr.set_frame_info(s.frame_info)
    tr.set_sky(s.sky)
    if vertex_motion:  # (first: inert until the two others are in force)
        tr.set_vertex_motion(True)
    if temporal:
        tr.set_temporal(True)
    if deform:
        tr.set_deformation(s.scene)
    return tr


def _first(s, frame_count=0):
    p = s.frame_params(0, 0)
    p.frameCount = frame_count
    return p


def _images(tr):
    a, n = tr.read_guides()
    return dict(accum=tr.read_accum(), albedo=a, normal=n, depth=tr.read_depth(), selection=tr.read_selection())


def _rc(call):
    with pytest.raises(ptmod.MiError) as e:
        call()
    return str(e.value)


def _yawed(s, cam, degrees, prev_view_proj=None):
    """Frame info of the scene's camera turned about its interest point; prevMVP = the given matrix (None: its own viewProjMatrix)."""
    a = np.radians(degrees)
    eye, center = np.array(cam.eye[:], np.float64), np.array(cam.center[:], np.float64)
    d = eye - center
    c, sn = np.cos(a), np.sin(a)
    eye = center + np.array([c * d[0] + sn * d[2], d[1], -sn * d[0] + c * d[2]])
    moved = capi.MiCamera()
    C.memmove(C.byref(moved), C.byref(cam), C.sizeof(cam))
    moved.eye[:] = [float(v) for v in eye]
    fi, _, _ = ptmod.camera_frame_info(moved, s.width, s.height)
    fi.flags = s.frame_info.flags
    fi.prevMVP[:] = fi.viewProjMatrix[:] if prev_view_proj is None else prev_view_proj
    return fi


def _node_arrays(scene):
    d = scene.desc.contents
    n = int(d.numRenderNodes)
    return (np.array([d.renderNodes[i].objectToWorld[:] for i in range(n)], np.float32), np.array([d.renderNodes[i].worldToObject[:] for i in range(n)], np.float32))


def _node_prims(scene):
    d = scene.desc.contents
    return np.array([d.renderNodes[i].renderPrimID for i in range(int(d.numRenderNodes))], np.int64)


def _translate_nodes(scene, shift):
    d = scene.desc.contents
    for i in range(int(d.numRenderNodes)):
        M = np.array(d.renderNodes[i].objectToWorld[:], np.float64).reshape(4, 4).T
        M[:3, 3] += shift
        d.renderNodes[i].objectToWorld[:] = [float(v) for v in M.T.reshape(-1).astype(np.float32)]
        d.renderNodes[i].worldToObject[:] = [float(v) for v in np.linalg.inv(M).T.reshape(-1).astype(np.float32)]


def _deform_ids(scene):
    return [int(p.renderPrimID) for p in du.prims(scene.deformation)]


def _indices(scene, pid):
    rp = scene.desc.contents.renderPrimitives[pid]
    return du.arr(rp.indices, int(rp.triangleCount) * 3, np.uint32).reshape(-1, 3)


def _run_sequence(path, vertex_motion, accel=None):
    """The sequence the tests share.  Pose 1: the clip at TA, camera still (deformation alone: the previous positions are the rest pose's).
    Pose 2: the clip at TB, a 2 degree camera yaw and every node moved by 0.1.  Pose 3: nothing updated, camera unchanged.  Pose 4: an update
    with the same tables, camera unchanged.  mi_pt_denoise_temporal (temporal stage alone) after each; everything is read back per pose."""
    s = _setup(path)
    tr = _tracer(s, vertex_motion)
    if accel is not None:
        tr.set_accel_update(accel)
    cam = s.scene.camera(0)
    ids = _deform_ids(s.scene)
    poses = []

    def pose(k, fi, prev_nodes):
        prev = {pid: tr.read_previous_positions(pid) for pid in ids} if vertex_motion else {pid: None for pid in ids}
        tr.set_frame_info(fi)
        tr.render_frame(_first(s, k))
        o2w, w2o = _node_arrays(s.scene)
        r = _images(tr)
        r.update(first_hit=tr.read_first_hit(), motion=tr.read_motion(), tri=tr.read_first_hit_triangle() if vertex_motion else None,
                 prims={pid: dict(indices=_indices(s.scene, pid), cur=tr.read_vertices(pid)[0], prev=prev[pid]) for pid in ids},
                 o2w=o2w, w2o=w2o, prev_o2w=prev_nodes, view_proj=np.array(fi.viewProjMatrix[:], np.float32), prev_mvp=np.array(fi.prevMVP[:], np.float32),
                 out=tr.denoise_temporal(iterations=0, **SIGMAS))
        poses.append(r)
        return o2w

    try:
        nodes = _node_arrays(s.scene)[0]
        fi1 = _yawed(s, cam, 0.0)
        assert s.scene.update_animation(0, TA)
        tr.update_from_scene(s.scene)
        nodes = pose(0, fi1, nodes)
        assert s.scene.update_animation(0, TB)
        _translate_nodes(s.scene, np.array([0.1, 0.0, 0.0]))
        tr.update_from_scene(s.scene)
        fi2 = _yawed(s, cam, 2.0, fi1.viewProjMatrix[:])
        nodes = pose(1, fi2, nodes)
        fi3 = _yawed(s, cam, 2.0)
        nodes = pose(2, fi3, nodes)
        tr.update_from_scene(s.scene)  # the same tables and matrices again
        pose(3, fi3, nodes)
        info = tr.accel_info()
    finally:
        tr.close()
    return dict(poses=poses, info=info, node_prims=_node_prims(s.scene), deform_ids=ids, extent=float(np.linalg.norm(np.subtract(*s.scene.bounds()[::-1]))))


@pytest.fixture(scope="module")
def seq_on(skinned):
    return _run_sequence(skinned, True)


@pytest.fixture(scope="module")
def seq_off(skinned):
    return _run_sequence(skinned, False)


def _ids(r):
    return np.ascontiguousarray(r["first_hit"][..., 3]).view(np.uint32)


def _deforming_pixels(seq, r):
    """Pixels whose first hit lies on a deforming render primitive (by the first-hit id)."""
    ids = _ids(r).astype(np.int64)
    mesh = (ids != 0) & (ids != tu.ID_INVALID)
    prim = np.where(mesh, seq["node_prims"][np.clip(ids - 1, 0, len(seq["node_prims"]) - 1)], -1)
    return mesh & np.isin(prim, seq["deform_ids"])


def _rigid(r):
    want, _ = tu.motion_numpy(r["first_hit"].reshape(-1, 4), r["o2w"], r["w2o"], r["prev_o2w"], r["view_proj"], r["prev_mvp"], W, H)
    return want.reshape(H, W, 3)


def _deformed(r):
    want, _, took = vu.vertex_motion_numpy(r["first_hit"].reshape(-1, 4), r["tri"].reshape(-1, 4), r["prims"], r["o2w"], r["w2o"], r["prev_o2w"], r["view_proj"],
                                           r["prev_mvp"], W, H)
    return want.reshape(H, W, 3), took.reshape(H, W)


# ---- the poses show what they are meant to show --------------------------------------------------------------------------------------
def test_the_two_poses_show_deforming_primitives_in_the_oracle(skinned):
    for time in (TA, TB):
        hs = _setup(skinned)
        assert hs.scene.update_animation(0, time)
        ids = _deform_ids(hs.scene)
        assert hs.scene.deform_on_host() == len(ids)
        sel = pu.render_oracle(hs, 1)["selection"].astype(np.int64)
        prim = np.where(sel > 0, _node_prims(hs.scene)[np.clip(sel - 1, 0, None)], -1)
        share = np.isin(prim, ids).mean()
        print("t = %.1f: %.1f %% of the pixels select deforming primitives" % (time, 100 * share))
        assert share >= 0.05, (time, share)


# ---- 1. off changes nothing ----------------------------------------------------------------------------------------------------------
def test_off_is_the_rigid_motion_and_on_changes_no_other_image(seq_on, seq_off):
    for k, (on, off) in enumerate(zip(seq_on["poses"], seq_off["poses"])):
        for name in ("accum", "albedo", "normal", "depth", "selection", "first_hit"):
            assert np.array_equal(on[name].view(np.uint32), off[name].view(np.uint32)), (k, name)
        want = _rigid(off)
        e_xy, e_z = np.abs(off["motion"][..., :2] - want[..., :2]).max(), np.abs(off["motion"][..., 2] - want[..., 2]).max()
        print("pose %d, off: |delta| to the rigid definition %.3g px (bound %.3g), depth %.3g" % (k + 1, e_xy, TOL_PX, e_z))
        assert e_xy <= TOL_PX and e_z <= TOL_Z, k
        assert np.array_equal(_ids(off), np.ascontiguousarray(off["motion"][..., 3]).view(np.uint32))


# ---- 2. the triangle record is the first hit -----------------------------------------------------------------------------------------
def test_triangle_record_names_the_first_hit(skinned, seq_on):
    # every primitive's indices, and the positions of those that do not deform (the deforming ones were read back at each pose)
    s = _setup(skinned)
    tr = ptmod.PathTracer(s.scene)
    num_prims = int(s.scene.desc.contents.numRenderPrimitives)
    file_prims = {pid: dict(indices=_indices(s.scene, pid), cur=tr.read_vertices(pid)[0]) for pid in range(num_prims)}
    tr.close()
    for k, r in enumerate(seq_on["poses"][:2]):
        ids, tri = _ids(r).astype(np.int64), r["tri"]
        mesh = (ids != 0) & (ids != tu.ID_INVALID)
        assert 0.3 < mesh.mean() < 1.0
        assert np.array_equal(tri[..., 0] == 0xFFFFFFFF, ~mesh)
        assert np.array_equal(tri[..., 0][mesh].astype(np.int64), seq_on["node_prims"][ids[mesh] - 1])
        prims = {pid: dict(p, cur=r["prims"][pid]["cur"] if pid in r["prims"] else p["cur"]) for pid, p in file_prims.items()}
        obj, known = vu.barycentric_point(tri.reshape(-1, 4), prims, "cur")
        assert np.array_equal(known.reshape(H, W), mesh)
        # objectToWorld x the barycentric sum of the resident positions is the recorded hit: a wrong vertex or a swapped barycentric is off
        # by a triangle's size
        fh, flat, worst = r["first_hit"].reshape(-1, 4), ids.reshape(-1), 0.0
        for i in np.nonzero(mesh.reshape(-1))[0]:
            world = (tu.mat(r["o2w"][flat[i] - 1]) @ np.append(obj[i], 1.0))[:3]
            worst = max(worst, float(np.abs(world - fh[i, :3]).max()))
        print("pose %d: |objectToWorld x barycentric sum - first hit| max %.3g (bound %.3g)" % (k + 1, worst, 1e-5 * seq_on["extent"]))
        assert worst <= 1e-5 * seq_on["extent"]


# ---- 3. the snapshot follows the rendered pose ---------------------------------------------------------------------------------------
def test_previous_positions_follow_the_rendered_pose(skinned):
    s = _setup(skinned)
    tr = _tracer(s)
    try:
        ids = _deform_ids(s.scene)
        cur = lambda: {pid: tr.read_vertices(pid)[0] for pid in ids}  # noqa: E731
        prev = lambda: {pid: tr.read_previous_positions(pid) for pid in ids}  # noqa: E731
        same = lambda a, b: all(np.array_equal(a[p].view(np.uint32), b[p].view(np.uint32)) for p in ids)  # noqa: E731

        def update(time):
            assert s.scene.update_animation(0, time)
            tr.update_from_scene(s.scene)
        rest = cur()
        assert same(prev(), rest)  # after enabling: previous == current
        update(TA)
        a = cur()
        assert not same(a, rest) and same(prev(), rest)
        tr.render_frame(_first(s, 0))
        assert same(prev(), a)
        update(1.0)
        update(TB)
        c = cur()
        assert not same(c, a) and same(prev(), a)  # two updates between two renders: still the last RENDERED pose
        tr.render_frame(_first(s, 1))
        assert same(prev(), c) and same(cur(), c)
        update(2.2)
        assert same(prev(), c) and not same(cur(), c)
        tr.render_frame(_first(s, 2))
        tr.render_frame(_first(s, 3))  # (no update since the last snapshot: nothing to copy, nothing changes)
        assert same(prev(), cur())
    finally:
        tr.close()


# ---- 4. the motion image against the float64 restatement -----------------------------------------------------------------------------
def test_motion_image_matches_the_float64_definition(seq_on):
    for k, r in enumerate(seq_on["poses"][:3]):
        want, took = _deformed(r)
        rigid = _rigid(r)
        on = _deforming_pixels(seq_on, r)
        e_xy, e_z = np.abs(r["motion"][..., :2] - want[..., :2]).max(), np.abs(r["motion"][..., 2] - want[..., 2]).max()
        gap = np.abs(r["motion"][..., :2] - rigid[..., :2])[on].max()
        print("pose %d: |delta| %.3g px (bound %.3g), depth %.3g; %d deforming pixels, %d on the deformed path, largest distance to the rigid motion %.2f px" % (
            k + 1, e_xy, TOL_PX, e_z, on.sum(), took.sum(), gap))
        assert e_xy <= TOL_PX and e_z <= TOL_Z, k
        assert np.array_equal(_ids(r), np.ascontiguousarray(r["motion"][..., 3]).view(np.uint32))
        assert on.mean() >= 0.05 and not (took & ~on).any()
        if k == 0:  # deformation alone: it is not the rigid motion
            assert gap > 1.0 and took.sum() > 0.5 * on.sum()
            assert (r["motion"][..., :2][~on] == 0.0).all()  # camera and nodes stood still
        if k == 1:
            assert np.abs(want[..., :2]).max() > 1.0 and took.sum() > 0.5 * on.sum()
        if k == 2:
            assert not took.any()


# ---- 5. still characters -------------------------------------------------------------------------------------------------------------
def test_still_characters_have_exactly_zero_motion(seq_on):
    for k in (2, 3):  # replayed with no update; replayed after an update with identical tables
        r = seq_on["poses"][k]
        assert _deforming_pixels(seq_on, r).mean() >= 0.05
        assert (r["motion"][..., :2] == 0.0).all(), k
        for pid, p in r["prims"].items():
            assert np.array_equal(p["prev"].view(np.uint32), p["cur"].view(np.uint32)), (k, pid)


# ---- 6. refit ------------------------------------------------------------------------------------------------------------------------
def test_refit_gives_the_same_motion_and_records(skinned, seq_on):
    refit = _run_sequence(skinned, True, accel="refit")
    assert refit["info"]["refits"] >= 1, refit["info"]
    for k, (a, b) in enumerate(zip(seq_on["poses"], refit["poses"])):
        assert np.array_equal(a["motion"].view(np.uint32), b["motion"].view(np.uint32)), k
        assert np.array_equal(a["tri"], b["tri"]), k


# ---- 7. state ------------------------------------------------------------------------------------------------------------------------
def test_refusals_memory_and_partition(skinned, assets):
    s = _setup(skinned)
    ids = _deform_ids(s.scene)
    d = s.scene.desc.contents
    num_prims = int(d.numRenderPrimitives)
    static = [p for p in range(num_prims) if p not in ids][0]
    slots = ((W + 63) // 64) * ((H + 63) // 64) * 64 * 64
    tr = _tracer(s, vertex_motion=False, temporal=False, deform=False)
    try:
        bare = tr.memory()
        assert "rc=-4" in _rc(tr.read_first_hit_triangle) and "rc=-4" in _rc(lambda: tr.read_previous_positions(ids[0]))
        tr.set_vertex_motion(True)  # inert: neither temporal nor deformation
        assert tr.memory()["rendererBytes"] == bare["rendererBytes"] and tr.memory()["sceneBytes"] == bare["sceneBytes"]
        tr.set_vertex_motion(False)
        tr.set_temporal(True)
        tr.set_deformation(s.scene)
        tr.render_frame(_first(s, 0))  # (the guide records exist from here on)
        base = tr.memory()
        tr.set_vertex_motion(True)
        now = tr.memory()
        assert now["rendererBytes"] - base["rendererBytes"] == 16 * slots
        verts = [int(d.renderPrimitives[p].vertexCount) for p in ids]
        assert now["sceneBytes"] - base["sceneBytes"] == sum((12 * v + 15) // 16 * 16 for v in verts) + 4 * len(ids) + 32 * num_prims
        assert "rc=-4" in _rc(tr.read_first_hit_triangle)  # no first-frame batch since it came into force
        assert "rc=-1" in _rc(lambda: tr.read_previous_positions(static))  # a primitive that does not deform
        tr.render_frame(_first(s, 1))
        assert (tr.read_first_hit_triangle()[..., 0] != 0xFFFFFFFF).mean() > 0.3
        tr.set_deformation(None)  # releases the previous positions; vertex motion is inert again
        assert "rc=-4" in _rc(lambda: tr.read_previous_positions(ids[0])) and "rc=-4" in _rc(tr.read_first_hit_triangle)
        m = tr.memory()
        assert m["rendererBytes"] == base["rendererBytes"] and m["sceneBytes"] == bare["sceneBytes"]
        tr.set_deformation(s.scene)
        assert tr.memory()["rendererBytes"] == now["rendererBytes"] and tr.memory()["sceneBytes"] == now["sceneBytes"]
        tr.set_vertex_motion(False)
        m = tr.memory()
        assert m["rendererBytes"] == base["rendererBytes"] and m["sceneBytes"] == base["sceneBytes"]
    finally:
        tr.close()
    # a 2-rank tile partition: only owned pixels carry records
    tr = _tracer(s, tile=(0, 2, 64))
    try:
        assert s.scene.update_animation(0, TA)
        tr.update_from_scene(s.scene)
        tr.render_frame(_first(s, 0))
        tri, fh = tr.read_first_hit_triangle(), tr.read_first_hit()
        mesh = np.ascontiguousarray(fh[..., 3]).view(np.uint32) != 0
        assert (tri[:, 64:] == 0xFFFFFFFF).all() and not mesh[:, 64:].any()
        assert mesh[:, :64].mean() > 0.3 and np.array_equal(tri[:, :64, 0] != 0xFFFFFFFF, mesh[:, :64])
    finally:
        tr.close()
    # a scene without deformers: the feature stays inert, the motion image is the one it renders without it
    b = pu.Setup(os.path.join(assets, "Box.glb"), 96, 64, max_depth=3, spp_per_frame=1, hdr_path=os.path.join(assets, "std_env.hdr"),
                 params_edit=lambda p: setattr(p, "flags", p.flags | capi.MI_PT_USE_OPTIX_DENOISER))
    cam = b.scene.camera(0)
    motion = {}
    for vm in (False, True):
        tr = _tracer(b, vertex_motion=vm)
        tr.set_environment(b.hdr)
        try:
            assert b.scene.deformation is None
            fi1 = _yawed(b, cam, 0.0)
            tr.set_frame_info(fi1)
            tr.render_frame(_first(b, 0))
            tr.set_frame_info(_yawed(b, cam, 2.0, fi1.viewProjMatrix[:]))
            tr.render_frame(_first(b, 1))
            motion[vm] = tr.read_motion()
            if vm:
                assert "rc=-4" in _rc(tr.read_first_hit_triangle)
        finally:
            tr.close()
    assert np.abs(motion[False][..., :2]).max() > 1.0 and np.array_equal(motion[False].view(np.uint32), motion[True].view(np.uint32))


# ---- 8. the temporal stage consumes the new motion -----------------------------------------------------------------------------------
def _stage_against_numpy(seq):
    """The temporal stage of the sequence's first two poses against temporal_util.reproject_numpy, with the tolerances and the cap on left-out
    pixels of test_gpu_temporal.py's test_temporal_stage_matches_numpy.  Returns the valid taps per pixel of pose 2."""
    hist, tainted, taps = None, None, None
    for k, r in enumerate(seq["poses"][:2]):
        hist, prepared, taps, margin, reads = tu.reproject_numpy(r["accum"], r["albedo"], r["normal"], r["depth"], r["motion"], hist, PARAMS, tainted)
        tainted = (margin < 1e-3) | reads
        assert tainted.mean() <= 0.005, (k, tainted.mean())
        want = tu.svgf_filter_numpy(prepared, r["accum"], r["albedo"], r["normal"], r["depth"], 0, SIGMAS["sigmaLuminance"], SIGMAS["sigmaNormal"], SIGMAS["sigmaDepth"])
        ok = ~tainted
        err = np.abs(r["out"][..., :3] - want[..., :3])[ok]
        scale, peak = np.abs(want[..., :3]).mean(), np.abs(want[..., :3]).max()
        print("pose %d: q99.9 %.3g (bound %.3g), max %.3g (bound %.3g), left out %.2f %%, taps 0/1-3/4: %d %d %d" % (
            k + 1, np.quantile(err, 0.999), 2e-3 * scale, err.max(), 5e-2 * peak, 100 * tainted.mean(), (taps == 0).sum(), ((taps > 0) & (taps < 4)).sum(), (taps == 4).sum()))
        assert np.quantile(err, 0.999) <= 2e-3 * scale and err.max() <= 5e-2 * peak, k
        assert np.array_equal(r["out"][..., 3], r["accum"][..., 3])
    return taps


def test_temporal_stage_consumes_the_vertex_motion(seq_on, seq_off):
    taps_on = _stage_against_numpy(seq_on)
    taps_off = _stage_against_numpy(seq_off)
    on = _deforming_pixels(seq_on, seq_on["poses"][1])
    print("pose 2, deforming pixels whose history resets (0 valid taps): rigid motion %.1f %%, vertex motion %.1f %% of %d" % (
        100 * (taps_off[on] == 0).mean(), 100 * (taps_on[on] == 0).mean(), on.sum()))
    assert (taps_on[on] > 0).any()


# ---- 9. the app ----------------------------------------------------------------------------------------------------------------------
def test_headless_app_plays_the_skinned_clip_with_vertex_motion(tmp_path, skinned):
    out = tmp_path / "vertex_motion.png"
    r = subprocess.run([os.path.join(ROOT, "vk_gltf_renderer_amd", "lib", "mi_gltf_renderer"), "--headless", "--size", "160", "96", "--scenefile", skinned,
                        "--ptSamples", "1", "--ptAdaptiveSampling", "0", "--ptMaxDepth", "3", "--frames", "6", "--maxFrames", "100", "--animStep", "0.1",
                        "--temporal", "1", "--vertexMotion", "1", "--output", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DENOISER passes=6 final_image=denoised temporal vertex-motion" in r.stdout, r.stdout[-800:] + r.stderr[-400:]
    assert out.exists() and out.stat().st_size > 1000
