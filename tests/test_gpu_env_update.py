"""Environment updates on the device (mi_pt_update_environment / mi_pt_update_environment_device / mi_pt_read_environment;
csrc/device/env_update.hip): for every size and pattern of tests/env_update_util.py the resident table is a valid alias table of the map's
distribution within the derived bounds written there, rgb / integral / pdf agree with the host route (mi_hdr_from_pixels) bit for bit / within
1 / within 2 float ulp, the bytes are the same on every call and from either form, and -- for the small sizes -- equal those of
tests/golden/env_update_cases.npz, which the host restatement of the same passes made (IEEE double in one fixed order on both sides).  An
updated instance renders bit for bit like a fresh instance given the read-back tables; a view of the sky alone like an instance fed by the
host route.  Every refusal leaves everything unchanged.

Convergence (test_renders_converge_like_the_host_table): the device's table and the host's are different tables of one distribution, so two
renders differ by noise.  rel-L2(device-table render, host-table render) may be at most 1.5 x rel-L2(host-table render, host-table render with
frameCount offset by 64), the reference's own noise floor; 1.5 absorbs the variance of the L2 estimate at 2 304 pixels.  Measured on one
MI355X: see LABNOTES.md ("Environment updates")."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import env_update_util as eu
import parity_util as pu
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

pytestmark = pytest.mark.gpu
ROOT = eu.ROOT
BOX = os.path.join(ROOT, "assets", "Box.glb")
CASES = eu.SMALL_CASES + ((1500, 750, "std_env"),)
MEMORY_KEYS = ("sceneBytes", "rendererBytes", "pathStateBytes")


def pixels_of(case):
    return eu.load_hdr_pixels() if case[2] == "std_env" else eu.make_pixels(*case)


def same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def render(tr, st, frames, batch=False, frame0=0):
    """`frames` frames from frame number frame0 (one mi_pt_render_frames batch, or one call each): accumulator, albedo and normal guides, selection."""
    tr.resize(st.width, st.height)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    if batch:
        p = st.frame_params(0, 0)
        p.frameCount = frame0
        p.flags |= capi.MI_PT_USE_OPTIX_DENOISER
        tr.render_frames(p, frames)
    else:
        total = 0
        for f in range(frames):
            p = st.frame_params(f, total)
            p.frameCount = frame0 + f
            p.flags |= capi.MI_PT_USE_OPTIX_DENOISER
            tr.render_frame(p)
            total += p.numSamples
    return (tr.read_accum(),) + tuple(tr.read_guides()) + (tr.read_selection(),)


@pytest.fixture(scope="module")
def plain(built):
    """Box.glb without an environment: the instances of the table tests."""
    return pu.Setup(BOX, 16, 16, max_depth=2)


@pytest.fixture(scope="module")
def tracer(plain):
    tr = ptmod.PathTracer(plain.scene)
    yield tr
    tr.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(eu.GOLDEN)


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=eu.case_id)
def test_table_is_valid_repeatable_and_matches_the_host_route(tracer, golden, case):
    px = pixels_of(case)
    n = px.shape[0] * px.shape[1]
    calls = tracer.environment_update_info()["calls"]
    tracer.update_environment(px)
    first = tracer.read_environment()
    eu.check_table(px, *first)
    eu.check_against_host_route(px, first[0], first[3])
    info = tracer.environment_update_info()
    assert info["calls"] == calls + 1 and info["launches"] == 6 and info["texelsSanitised"] == 0 and info["integral"] == first[3]
    assert info["lightTexels"] + info["heavyTexels"] == (n if first[3] > 0 else 0)
    assert 12 * n <= info["scratchBytes"]
    tracer.update_environment(px)
    assert same_bytes(tracer.read_environment(), first)  # a second call
    px4 = np.concatenate([px, np.full(px.shape[:2] + (1,), np.nan, np.float32)], -1)  # RGBA32F: staged inside the resident map, alpha ignored
    tracer.update_environment(px4)
    assert same_bytes(tracer.read_environment(), first)
    if case in eu.SMALL_CASES:
        same = eu.same_as_golden(golden, case, *first)
        assert all(same.values()), same


# ---- 2. the device form --------------------------------------------------------------------------------------------------------------------------
def test_device_form_with_torch_tensors(tmp_path):
    """In a process of its own (tests/env_update_device_child.py): torch brings its own copy of the HIP runtime, and the two libraries share one
    only when torch is loaded first.  For every size and pattern the child compares the bytes the device form leaves (RGB and RGBA tensors, a
    second call, a tensor that starts off a 16-byte boundary) with the host form's; it checks that NaN, -1 and +inf texels are counted, read
    back 0 and leave a valid table, that the host form refuses the same data with nothing changed, and the refusal of misaligned pointers."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "env_update_device_child.py"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "ENV_UPDATE_DEVICE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---- 3. rendering ----------------------------------------------------------------------------------------------------------------------------------
def test_updated_instance_renders_like_a_fresh_instance_with_the_same_tables(built):
    px = eu.gradient_with_patch()
    st = pu.Setup(BOX, 64, 64, max_depth=3, hdr_pixels=px)
    a, b = ptmod.PathTracer(st.scene), ptmod.PathTracer(st.scene)
    try:
        a.update_environment(px)
        tables = a.read_environment()
        env, keep = eu.make_environment(*tables)
        ptmod._check_pt(b._l.mi_pt_set_environment(b._p, C.byref(env)))
        del keep
        assert same_bytes(b.read_environment(), tables)
        got, want = render(a, st, 2), render(b, st, 2)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        assert np.isfinite(got[0]).all() and got[0][..., :3].max() > 0
        a.update_environment(np.full(px.shape, 0.01, np.float32))
        assert render(a, st, 2)[0].tobytes() != got[0].tobytes()  # (the environment lights the frame)
    finally:
        a.close()
        b.close()


def test_same_size_is_in_place_and_another_size_is_a_replacement(built):
    small, other, large = eu.make_pixels(64, 32, "tail"), eu.make_pixels(64, 32, "halves"), eu.make_pixels(65, 33, "halves")
    st = pu.Setup(BOX, 64, 64, max_depth=3, hdr_pixels=large)
    tr, fresh = ptmod.PathTracer(st.scene), ptmod.PathTracer(st.scene)
    try:
        m0 = tr.memory()
        tr.update_environment(small)
        m1 = tr.memory()
        scratch = tr.environment_update_info()["scratchBytes"]
        assert m1["sceneBytes"] == m0["sceneBytes"] + 64 * 32 * (16 + 8) and m1["rendererBytes"] == m0["rendererBytes"] + scratch
        tr.update_environment(other)
        assert all(tr.memory()[k] == m1[k] for k in MEMORY_KEYS)  # in place
        eu.check_table(other, *tr.read_environment())
        tr.update_environment(large)
        m2 = tr.memory()
        grown = tr.environment_update_info()["scratchBytes"]
        assert m2["sceneBytes"] == m0["sceneBytes"] + 65 * 33 * (16 + 8) and grown > scratch and m2["rendererBytes"] == m0["rendererBytes"] + grown
        fresh.update_environment(large)
        assert same_bytes(tr.read_environment(), fresh.read_environment())
        for g, w in zip(render(tr, st, 2), render(fresh, st, 2)):
            assert g.tobytes() == w.tobytes()
        tr.update_environment(small)  # back: the map shrinks, the scratch stays
        m3 = tr.memory()
        assert tr.environment_update_info()["scratchBytes"] == grown and m3["sceneBytes"] == m1["sceneBytes"]
        eu.check_table(small, *tr.read_environment())
        assert tr.environment_update_info()["calls"] == 4 and tr.environment_update_info()["texelsWritten"] == 3 * 64 * 32 + 65 * 33
    finally:
        tr.close()
        fresh.close()


def test_a_view_of_the_sky_alone_equals_the_host_route(built):
    px = eu.make_pixels(65, 33, "tail")
    probe = ptmod.Scene(BOX)
    cam = probe.camera(0)
    probe.close()
    cam.eye[:], cam.center[:], cam.up[:] = (0.0, 0.0, 50.0), (0.0, 30.0, 100.0), (0.0, 1.0, 0.0)  # the box lies behind the camera
    st = pu.Setup(BOX, 64, 64, max_depth=3, hdr_pixels=px, camera=cam)
    a, b = ptmod.PathTracer(st.scene), ptmod.PathTracer(st.scene)
    try:
        a.update_environment(px)
        b.set_environment(st.hdr)
        got, want = render(a, st, 2), render(b, st, 2)
        assert (got[3] == 0).all() and (want[3] == 0).all()  # nothing but sky
        assert got[0].tobytes() == want[0].tobytes()  # misses read rgb only
        assert got[0][..., :3].max() > 0 and len(np.unique(got[0][..., :3])) > 16
    finally:
        a.close()
        b.close()


def test_renders_converge_like_the_host_table(built):
    px = eu.gradient_with_patch()
    st = pu.Setup(BOX, 48, 48, max_depth=3, hdr_pixels=px)
    dev, host = ptmod.PathTracer(st.scene), ptmod.PathTracer(st.scene)
    try:
        dev.update_environment(px)
        host.set_environment(st.hdr)
        d = render(dev, st, 64, batch=True)[0][..., :3].astype(np.float64)
        h = render(host, st, 64, batch=True)[0][..., :3].astype(np.float64)
        h2 = render(host, st, 64, batch=True, frame0=64)[0][..., :3].astype(np.float64)
    finally:
        dev.close()
        host.close()
    rel = lambda x, ref: float(np.sqrt(((x - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum()))  # noqa: E731
    device_vs_host, floor = rel(d, h), rel(h2, h)
    print("convergence: rel-L2(device table, host table) = %.5f, rel-L2(host table, host table at frameCount + 64) = %.5f, ratio %.3f"
          % (device_vs_host, floor, device_vs_host / floor))
    assert floor > 0 and device_vs_host <= 1.5 * floor, (device_vs_host, floor)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------
def _raw(tr, width, height, channels, pixels, flags=0, reserved=(0, 0), device=False):
    u = capi.MiPtEnvironmentUpdate()
    u.width, u.height, u.channels, u.flags = width, height, channels, flags
    u.pixels = pixels if pixels is None or isinstance(pixels, int) else pixels.ctypes.data
    u.reserved[0], u.reserved[1] = reserved
    fn = tr._l.mi_pt_update_environment_device if device else tr._l.mi_pt_update_environment
    return fn(tr._p, C.byref(u))


def test_refusals_leave_everything_unchanged(plain):
    tr = ptmod.PathTracer(plain.scene)
    try:
        with pytest.raises(ptmod.MiError) as e:
            tr.read_environment()
        assert "rc=-4" in str(e.value)
        assert tr._l.mi_pt_read_environment(tr._p, None, None, None, None, None) == -4
        px = eu.make_pixels(5, 3, "tail")
        px4 = np.concatenate([px, np.full((3, 5, 1), np.nan, np.float32)], -1)
        tr.update_environment(eu.make_pixels(5, 3, "halves"))
        state = lambda: ([np.asarray(x).tobytes() for x in tr.read_environment()], tr.environment_update_info(), [tr.memory()[k] for k in MEMORY_KEYS])  # noqa: E731
        before = state()
        bad = {}
        for name, value in (("nan", np.nan), ("inf", np.inf), ("negative", -1.0e-30), ("minus inf", -np.inf)):
            bad[name] = px.copy()
            bad[name][1, 2, 1] = value
        bad4 = px4.copy()
        bad4[2, 4, 0] = np.nan
        refused = {
            "zero width": lambda: _raw(tr, 0, 3, 3, px), "negative height": lambda: _raw(tr, 5, -3, 3, px),
            "too many texels": lambda: _raw(tr, 8193, 8192, 3, px), "overflowing size": lambda: _raw(tr, 2 ** 31 - 1, 2 ** 31 - 1, 3, px),
            "two channels": lambda: _raw(tr, 5, 3, 2, px), "five channels": lambda: _raw(tr, 5, 3, 5, px),
            "unknown flag": lambda: _raw(tr, 5, 3, 3, px, flags=1), "reserved 0": lambda: _raw(tr, 5, 3, 3, px, reserved=(1, 0)),
            "reserved 1": lambda: _raw(tr, 5, 3, 3, px, reserved=(0, 7)), "null pixels": lambda: _raw(tr, 5, 3, 3, None),
            "null update": lambda: tr._l.mi_pt_update_environment(tr._p, None), "null update, device": lambda: tr._l.mi_pt_update_environment_device(tr._p, None),
            "rgba with a nan colour": lambda: _raw(tr, 5, 3, 4, bad4),
            # the device form checks the alignment before anything else is done with the address
            "misaligned rgb": lambda: _raw(tr, 5, 3, 3, 0x7f0000001002, device=True), "misaligned rgba": lambda: _raw(tr, 5, 3, 4, 0x7f0000001008, device=True),
            "null pixels, device": lambda: _raw(tr, 5, 3, 3, None, device=True),
        }
        refused.update({name: (lambda a=a: _raw(tr, 5, 3, 3, a)) for name, a in bad.items()})
        for why, call in refused.items():
            assert call() == -1, why
            assert state() == before, why
        assert _raw(tr, 5, 3, 4, px4) == 0  # (NaN in the input alpha is nobody's business)
        eu.check_table(px, *tr.read_environment())
        # the frame queue is flushed: a frame recorded before an update shows the old map
        st = pu.Setup(BOX, 16, 16, max_depth=2, hdr_pixels=px)
        old = render(tr, st, 1)[0].copy()
        tr.set_frame_queue(4)
        p = st.frame_params(0, 0)
        p.flags |= capi.MI_PT_USE_OPTIX_DENOISER
        tr.render_frame(p)  # (held back)
        tr.update_environment(eu.make_pixels(5, 3, "constant"))
        assert tr.read_accum().tobytes() == old.tobytes()
        tr.set_frame_queue(1)
        assert render(tr, st, 1)[0].tobytes() != old.tobytes()
    finally:
        tr.close()
