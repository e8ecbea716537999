"""mi_gltf_renderer --projection: the headless app makes the camera rays of a panorama or a fisheye itself (mi_camera_rays, one jittered set per
frame in flight) and binds them (mi_pt_set_camera_rays).  Its image is the one the Python route renders with the same rays bound -- compared on
the codes of the RGBE file the app writes (its HDR output: the accumulator before tonemapping, 8-bit mantissas) -- and --temporal 1 is refused.

The app's jitter ("Caller-supplied camera rays"): set 0 is the pixel centre; set k > 0 takes draws 2k and 2k + 1 of the PCG
stream that starts at state 0x9E3779B9 -- state = state * 747796405 + 2891336453, the library's output permutation, top 24 bits / 2^24."""
import os
import subprocess

import numpy as np
import pytest

import parity_util as pu
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(capi.LIB_DIR, "mi_gltf_renderer")
W, H, FRAMES = 64, 32, 3
M32 = 0xffffffff
F32 = np.float32


def _run(args):
    if not os.path.exists(EXE):
        pytest.skip("mi_gltf_renderer not built (run __graft_entry__.build())")
    env = dict(os.environ, LD_LIBRARY_PATH=capi.LIB_DIR + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=env, timeout=300)


def app_jitter(num_sets):
    state, out = 0x9E3779B9, []
    for k in range(num_sets):
        pair = []
        for _ in range(2):
            state = (state * 747796405 + 2891336453) & M32
            word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
            pair.append((((word >> 22) ^ word) >> 8) / 16777216.0)
        out.append((0.5, 0.5) if k == 0 else tuple(pair))
    return np.asarray(out, F32)


def rgbe(img):
    """GltfRenderer::saveHdr's codes of an RGBA float image (flat scanlines; float32 arithmetic, truncation)."""
    rgb = np.where(np.isfinite(img[..., :3]) & (img[..., :3] > 0), img[..., :3], 0).astype(F32)
    m = rgb.max(-1)
    mant, e = np.frexp(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (mant.astype(F32) * F32(256)) / m
    out = np.zeros(img.shape[:2] + (4,), np.uint8)
    ok = m >= F32(1e-32)
    q = np.minimum(F32(255), rgb * s[..., None])
    out[..., :3] = np.where(ok[..., None], q, 0).astype(np.uint8)
    out[..., 3] = np.where(ok, np.clip(e + 128, 0, 255), 0).astype(np.uint8)
    nudge = (out[:, 0, 0] == 2) & (out[:, 0, 1] == 2) & (out[:, 0, 2] < 128)
    out[nudge, 0, 1] = 3
    return out


def test_app_jitter_is_the_documented_stream():
    j = app_jitter(5)
    assert j.shape == (5, 2) and tuple(j[0]) == (0.5, 0.5) and ((j >= 0) & (j < 1)).all() and len({tuple(x) for x in j}) == 5
    assert (app_jitter(3) == j[:3]).all()  # set k does not depend on how many sets there are
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "0x9E3779B9" in doc and "--projection" in doc and "--fisheyeFov" in doc


def test_projection_refuses_temporal_and_unknown_names(assets):
    base = ["--headless", "--size", str(W), str(H), "--scenefile", os.path.join(assets, "Box.glb"), "--frames", "1"]
    r = _run(base + ["--projection", "fisheye", "--temporal", "1"])
    assert r.returncode != 0 and "cannot be combined with --temporal 1" in r.stderr, r.stderr
    r = _run(base + ["--projection", "cylinder"])
    assert r.returncode != 0 and "--projection must be perspective, equirect or fisheye" in r.stderr, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("projection,fov", [("equirect", 180.0), ("fisheye", 220.0)])
def test_headless_projection_is_the_python_route(tmp_path, assets, projection, fov):
    out = tmp_path / "pano.hdr"
    glb, hdr = os.path.join(assets, "Box.glb"), os.path.join(assets, "std_env.hdr")
    r = _run(["--headless", "--size", str(W), str(H), "--scenefile", glb, "--hdrfile", hdr, "--envSystem", "1", "--frames", str(FRAMES), "--maxFrames", str(FRAMES),
              "--ptSamples", "1", "--ptAdaptiveSampling", "0", "--ptMaxDepth", "4", "--framesInFlight", str(FRAMES), "--projection", projection,
              "--fisheyeFov", str(fov), "--output", str(out)])
    assert r.returncode == 0, r.stdout + r.stderr
    data = out.read_bytes()
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W)
    assert data.startswith(head) and len(data) == len(head) + W * H * 4
    saved = np.frombuffer(data[len(head):], np.uint8).reshape(H, W, 4)
    st = pu.Setup(glb, W, H, hdr_path=hdr, max_depth=4)
    rays, angle = ptmod.camera_rays(st.scene.camera(0), W, H, projection, fov=fov, jitter=app_jitter(FRAMES))
    st.params.pixelAngle = angle
    tr = ptmod.PathTracer(st.scene)
    tr.set_environment(st.hdr)
    tr.resize(W, H)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    tr.set_camera_rays(rays, unit=True)
    tr.render_frame(st.frame_params(0, 0))
    tr.render_frames(st.frame_params(1, 1), FRAMES - 1)
    want = tr.read_accum()
    tr.close()
    assert (want[..., :3] > 0).any() and np.isfinite(want).all()
    if projection == "fisheye":
        assert (want[0, 0] == 0).all() and (saved[0, 0] == 0).all()  # outside the image circle: no path
    assert (saved == rgbe(want)).all(), int((saved != rgbe(want)).sum())
    # and it is not the perspective image
    plain = tmp_path / "plain.hdr"
    assert _run(["--headless", "--size", str(W), str(H), "--scenefile", glb, "--hdrfile", hdr, "--envSystem", "1", "--frames", str(FRAMES), "--maxFrames", str(FRAMES),
                 "--ptSamples", "1", "--ptAdaptiveSampling", "0", "--ptMaxDepth", "4", "--output", str(plain)]).returncode == 0
    assert plain.read_bytes() != data
