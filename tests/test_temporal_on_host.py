"""CPU tier of the motion vectors and the temporal reprojection: csrc/device/pt_temporal.h (motionRecord, reprojectPixel) compiled for
the host through tests/host_shim (g++ -ffp-contract=off) and diffed against the float64 numpy restatements of tests/temporal_util.py,
which are written from the reference's lines and from Schied et al. 2017, not from the header.  Plus the public surface: the five entry
points in the header, the binding and the built library, and the ABI version."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, P = C.c_float, C.POINTER
ENTRY_POINTS = ("mi_pt_read_first_hit", "mi_pt_set_temporal", "mi_pt_read_motion", "mi_pt_denoise_temporal", "mi_pt_reset_history")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("temporal_shim") / "libtemporal_on_host.so")
    d = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-I" + d, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"), "-o", out, os.path.join(d, "temporal_on_host.cpp")], check=True)
    L = C.CDLL(out)
    L.dev_motion_records.argtypes = [C.c_int, P(F), C.c_void_p, P(F), C.c_int, P(F), P(F), F, F, P(F)]
    L.dev_motion_records.restype = None
    L.dev_reproject_image.argtypes = [C.c_int, C.c_int, P(F), C.c_int, P(F), P(F), P(F), P(F), P(F), P(P(F)), P(P(F)), P(F), P(C.c_int)]
    L.dev_reproject_image.restype = None
    return L


def fp(a):
    return a.ctypes.data_as(P(F))


# ---- motion vectors ------------------------------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _rigid(rng, max_angle, max_shift):
    M = np.eye(4)
    M[:3, :3] = _rotation(rng.normal(size=3), rng.uniform(-max_angle, max_angle))
    M[:3, 3] = rng.uniform(-max_shift, max_shift, 3)
    return M


def _view_proj(eye, yaw, pitch, fov_deg, aspect, near=0.1, far=1000.0):
    R = _rotation(np.array([1.0, 0, 0]), pitch) @ _rotation(np.array([0, 1.0, 0]), yaw)  # world -> view rotation
    V = np.eye(4)
    V[:3, :3] = R
    V[:3, 3] = -R @ eye
    f = 1.0 / np.tan(np.radians(fov_deg) / 2)
    Pm = np.array([[f / aspect, 0, 0, 0], [0, -f, 0, 0], [0, 0, far / (near - far), near * far / (near - far)], [0, 0, -1, 0]])
    return Pm @ V


def _cm(M):
    """4x4 matrix -> 16 column-major float32."""
    return np.ascontiguousarray(M.T, np.float32).reshape(16)


def _run_motion(shim, fh, o2w, w2o, prev, vp, pm, W, H):
    nodes = np.zeros((len(o2w), 34), np.float32)  # MiGltfRenderNode: objectToWorld, worldToObject, materialID, renderPrimID
    nodes[:, :16], nodes[:, 16:32] = o2w, w2o
    fh = np.ascontiguousarray(fh, np.float32)
    prev = np.ascontiguousarray(prev, np.float32)
    out = np.zeros((len(fh), 4), np.float32)
    shim.dev_motion_records(len(fh), fp(fh), nodes.ctypes.data_as(C.c_void_p), fp(prev), len(o2w), fp(vp), fp(pm), W, H, fp(out))
    return out


def _motion_case(seed):
    """2 000 points under seeded rigid node motions and two cameras: 1 600 surface points on 8 nodes (3 of which stand still), 400 sky
    directions.  Camera near the origin and points at 4 .. 40 units inside both frusta, so that both clip w stay >= 0.1 by construction."""
    rng = np.random.default_rng(seed)
    W, H = 1920.0, 1080.0
    cam = dict(eye=rng.uniform(-1, 1, 3), yaw=rng.uniform(-0.3, 0.3), pitch=rng.uniform(-0.2, 0.2))
    vp = _view_proj(cam["eye"], cam["yaw"], cam["pitch"], 45.0, W / H)
    pm = _view_proj(cam["eye"] + rng.uniform(-0.2, 0.2, 3), cam["yaw"] + np.radians(2.0), cam["pitch"] - np.radians(1.0), 45.0, W / H)
    K = 8
    cur = [_rigid(rng, 0.8, 0.5) for _ in range(K)]
    prev = [c if k < 3 else _rigid(rng, np.radians(5.0), 0.3) @ c for k, c in enumerate(cur)]
    o2w = np.stack([_cm(c) for c in cur])
    w2o = np.stack([_cm(np.linalg.inv(c)) for c in cur])
    pv = np.stack([_cm(c) for c in prev])
    ndc = rng.uniform(-0.8, 0.8, (2000, 2))
    dist = rng.uniform(4.0, 40.0, 2000)
    inv = np.linalg.inv(vp)
    far_pt = (inv @ np.concatenate([ndc, np.full((2000, 1), 0.5), np.ones((2000, 1))], 1).T).T
    far_pt = far_pt[:, :3] / far_pt[:, 3:4]
    d = far_pt - cam["eye"]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    fh = np.zeros((2000, 4), np.float32)
    fh[:1600, :3] = cam["eye"] + d[:1600] * dist[:1600, None]
    fh[1600:, :3] = d[1600:]
    ids = np.zeros(2000, np.uint32)
    ids[:1600] = rng.integers(1, K + 1, 1600)
    fh[:, 3] = ids.view(np.float32)
    return fh, o2w, w2o, pv, _cm(vp), _cm(pm), W, H


def test_motion_vector_matches_the_reference_definition(shim):
    fh, o2w, w2o, pv, vp, pm, W, H = _motion_case(20251017)
    got = _run_motion(shim, fh, o2w, w2o, pv, vp, pm, W, H)
    want, clipw = tu.motion_numpy(fh, o2w, w2o, pv, vp, pm, W, H)
    assert (np.abs(clipw) >= 0.1).all(), "the generator left a point outside the stated condition (both clip w >= 0.1)"
    err = np.abs(got[:, :2] - want[:, :2])
    print("motion |delta| px: max %.3g, surface %.3g, sky %.3g" % (err.max(), err[:1600].max(), err[1600:].max()))
    # ~ten fp32 roundings on pixel coordinates up to 1e3 (1e3 * 10 * 6e-8 = 6e-4 worst case, ~1e-4 typical), bound set with that margin
    assert err.max() <= 1e-3
    assert np.abs(got[:1600, 2] - want[:1600, 2]).max() <= 1e-6 and (got[1600:, 2] == 1.0).all()
    assert np.array_equal(got[:, 3].view(np.uint32), fh[:, 3].view(np.uint32))
    assert np.abs(want[:, :2]).max() > 10.0  # (the case really moves)


def test_motion_is_exactly_zero_when_nothing_moved(shim):
    fh, o2w, w2o, pv, vp, pm, W, H = _motion_case(7)
    got = _run_motion(shim, fh, o2w, w2o, o2w, vp, vp, W, H)  # identical cameras and matrices
    assert (got[:, :2] == 0.0).all()
    # ... and the invalid id: zero motion, the id kept invalid
    bad = fh[:4].copy()
    bad[:, 3] = np.array([0xFFFFFFFF] * 4, np.uint32).view(np.float32)
    got = _run_motion(shim, bad, o2w, w2o, pv, vp, pm, W, H)
    assert (got[:, :2] == 0.0).all() and (got[:, 3].view(np.uint32) == 0xFFFFFFFF).all()


def test_sky_ignores_camera_translation(shim):
    fh, o2w, w2o, pv, vp, pm, W, H = _motion_case(11)
    moved = vp.copy()
    moved[12:16] += np.array([0.37, -1.25, 0.11, 0.6], np.float32)  # a translation of the camera changes the fourth column alone
    got = _run_motion(shim, fh, o2w, w2o, o2w, vp, moved, W, H)
    assert (got[1600:, :2] == 0.0).all()
    assert np.abs(got[:1600, :2]).max() > 1.0  # surfaces do move


# ---- reprojection --------------------------------------------------------------------------------------------------------------------
PARAMS = dict(alpha=0.2, momentsAlpha=0.2, maxHistory=32.0, normalCos=0.9, depthTolerance=0.1)
GW, GH = 48, 32


def _gbuffer(pose, rng):
    """Sky rows on top (id 0), two background planes of one node at different depths (the camera pans by a fraction of a pixel), and a
    10 x 10 square of a second node that moves 3.5 px per pose."""
    ids = np.full((GH, GW), 1, np.uint32)
    depth = np.where(np.arange(GW)[None, :] < 24, 0.95, 0.99) * np.ones((GH, 1))
    normal = np.zeros((GH, GW, 4), np.float32)
    normal[..., 2] = 1.0
    motion = np.zeros((GH, GW, 4), np.float32)
    motion[..., 0], motion[..., 1] = 0.25, 0.5
    motion[..., 2] = depth
    ids[:4], depth[:4] = 0, 1.0
    normal[:4] = 0.0
    motion[:4, :, 2] = 1.0
    x0 = 4 + int(np.floor(3.5 * pose))
    sq = (slice(12, 22), slice(x0, x0 + 10))
    ids[sq], depth[sq] = 2, 0.9
    normal[sq] = (0.0, 0.6, 0.8, 0.0)
    # the square's points were 3.5 px to the left; its pixel origin advances by 3 or 4, the rest is sub-pixel motion
    motion[sq] = (-3.5, 0.0, 0.9, 0.0)
    motion[..., 3] = ids.view(np.float32)
    albedo = np.zeros((GH, GW, 4), np.float32)
    albedo[..., :3] = np.where(ids[..., None] == 2, (0.8, 0.3, 0.2), (0.4, 0.5, 0.6))
    albedo[..., 3] = ids != 0
    base = np.where(ids == 2, 0.7, np.where(ids == 1, 0.3, 1.5))
    color = np.zeros((GH, GW, 4), np.float32)
    color[..., :3] = base[..., None] * rng.uniform(0.2, 1.8, (GH, GW, 3))
    color[..., 3] = albedo[..., 3]
    return color, albedo, normal, depth.astype(np.float32), motion


def test_reprojection_matches_numpy_per_pixel(shim):
    rng = np.random.default_rng(424242)
    consts = np.array([PARAMS[k] for k in ("alpha", "momentsAlpha", "maxHistory", "normalCos", "depthTolerance")], np.float32)
    dev = [[np.zeros((GH, GW, 4), np.float32) for _ in range(3)] for _ in range(2)]
    ptrs = [(P(F) * 3)(*[fp(a) for a in s]) for s in dev]
    hist, cur = None, 0
    share = {"reset": 0.0, "partial": 0.0, "full": 0.0}
    for pose in range(6):
        color, albedo, normal, depth, motion = _gbuffer(pose, rng)
        illum, taps = np.zeros((GH, GW, 4), np.float32), np.zeros((GH, GW), np.int32)
        shim.dev_reproject_image(GW, GH, fp(consts), int(hist is not None), fp(color), fp(albedo), fp(normal), fp(depth), fp(motion), ptrs[cur], ptrs[cur ^ 1],
                                 fp(illum), taps.ctypes.data_as(P(C.c_int)))
        hist, want, wtaps, margin, _ = tu.reproject_numpy(color, albedo, normal, depth, motion, hist, PARAMS)
        cur ^= 1
        got_illum, got_mom, got_nrm = dev[cur]
        assert margin.min() > 1e-2  # (the synthetic G-buffer keeps every decision far from its threshold)
        assert np.array_equal(taps, wtaps), pose
        tol = dict(rtol=2e-5, atol=2e-6)
        assert np.allclose(illum[..., :3], want[..., :3], **tol) and np.allclose(got_illum[..., :3], hist["illum"], **tol)
        assert np.allclose(got_illum[..., 3], hist["h"], **tol)
        assert np.allclose(got_mom[..., 0], hist["m1"], **tol) and np.allclose(got_mom[..., 1], hist["m2"], **tol)
        assert np.array_equal(got_mom[..., 2], depth) and np.array_equal(got_mom[..., 3].view(np.uint32), hist["id"])
        assert np.array_equal(got_nrm[..., :3], normal[..., :3])
        # variance: a difference of two nearly equal moments -- absolute tolerance at the scale of the second moment
        assert np.abs(illum[..., 3] - want[..., 3]).max() <= 1e-5 * max(1.0, hist["m2"].max())
        if pose:
            n = float(GW * GH)
            share["reset"] = max(share["reset"], (wtaps == 0).sum() / n)
            share["partial"] = max(share["partial"], ((wtaps >= 1) & (wtaps <= 3)).sum() / n)
            share["full"] = max(share["full"], (wtaps == 4).sum() / n)
        if pose == 0:
            assert (wtaps == 0).all() and (hist["h"] == 1.0).all()
    print("tap classes, largest share over poses 1..5:", share)
    assert min(share.values()) >= 0.02, share
    # a pixel with h >= 4 uses the temporal variance (and that is not what the spatial estimate gives there)
    old = hist["h"] >= 4.0
    assert old.mean() > 0.2
    temporal = np.maximum(0.0, hist["m2"] - hist["m1"] ** 2)
    il = color[..., :3].astype(np.float64) / tu.demodulator(albedo)
    spatial = tu.spatial_variance(il, albedo, normal)
    assert np.abs(illum[..., 3][old] - temporal[old]).max() <= 1e-5 * max(1.0, hist["m2"].max())
    assert np.abs(temporal[old] - spatial[old]).mean() > 1e-3


# ---- public surface ------------------------------------------------------------------------------------------------------------------
def test_temporal_entry_points_are_declared_bound_and_exported(built):
    from vk_gltf_renderer_amd import _capi as capi
    header = open(os.path.join(ROOT, "include", "mi_pt.h")).read()
    assert re.search(r"#define MI_PT_ABI_VERSION 9\b", header)
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vk_gltf_renderer_amd", "lib", "libmi_pt.so")], check=True,
                              capture_output=True, text=True).stdout
    for name in ENTRY_POINTS + ("mi_pt_default_temporal",):
        assert re.search(r"MI_PT_API\s+\w+\s+%s\(" % name, header), name
        assert name in capi.PT_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    assert capi.MI_PT_ABI_VERSION == 9 and capi.pt_lib().mi_pt_abi_version() == 9
    tp = capi.MiPtTemporalParams()
    capi.pt_lib().mi_pt_default_temporal(C.byref(tp))
    assert abs(tp.alpha - 0.2) < 1e-7 and abs(tp.momentsAlpha - 0.2) < 1e-7 and tp.maxHistory >= 4.0
