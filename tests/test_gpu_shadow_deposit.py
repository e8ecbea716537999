"""The any-hit shadow walks of opaque and alpha-tested scenes (k_trace_shadow MODE 0 / 1) add an unoccluded ray's term to the path's radiance record where the ray
ends -- three float atomics without a returned value (pt_scene.h: shadowDepositAdd) -- instead of leaving every ray's outcome in its queue entry for a pass of its
own (k_shadow_resolve<false>, which now runs for shadow-catcher probes only).  MI_PT_SHADOW_DEPOSIT=0 selects the pass for every ray, as before: a second
implementation of the same sum.  A path has at most one shadow ray per bounce and the record is its own, so each component gets one rounded add either way and the
images must agree BIT FOR BIT; every case renders its frames with the switch on and off, compares accumulator, depth and selection byte for byte and the path-level
counters, and holds the switch-on image against the CPU oracle with the tolerance of the parity test of its scene class (tests/test_gpu_parity.py).

The switch is read when the tracer is created.  Cases 1, 2 and 5 force the side-stream schedule (MI_PT_OVERLAP_MIN_TRIS=0: the shadow stage of a small batch runs next
to the following bounce's closest-hit walk); case 3 runs batches of 64 (pixel-major slots) and single frames on one stream; the catcher frames of case 4 keep the path
state by slot and one stream by themselves.

The last test asks the part what its memory-side float add computes (tests/device_kat/kat_atomic_deposit.hip): word-for-word numpy's float32 add wherever operands
and result are normal, zero or infinite; the denormal rows are printed (LABNOTES.md, "The shadow walk deposits its own results", records what they showed)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import device_kat_lib as kat
import parity_util as pu
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu

COUNTERS = ("cameraPaths", "segments", "surfaceHits", "shadowRays", "textureTaps")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _render(s, frames, deposit, env=None, **kw):
    with _env(MI_PT_SHADOW_DEPOSIT=deposit, **(env or {})):
        return pu.render_gpu(s, frames, **kw)


def _same_images(on, off, what):
    for k in ("accum", "depth", "selection"):
        assert on[k].tobytes() == off[k].tobytes(), (what, k, int((on[k] != off[k]).sum()))


def _same(on, off, what):
    _same_images(on, off, what)
    for k in COUNTERS:  # (path level: the walks' node / triangle counts depend on which rays a persistent wave picks up together)
        assert on["stats"][k] == off["stats"][k], (what, k)
    assert on["stats"]["shadowRays"] > 0, what


def _check(o, g, what, rel_l2=1e-3, within_1e2=0.99, within_1e4=0.97, counter_rel=2e-3, depth_tol=2e-6, alpha_tol=5e-4):
    """The bounds of tests/test_gpu_parity.py::_check."""
    m = pu.compare_images(o["accum"], g["accum"])
    print("PARITY", what, "rel_l2 %.3e (bound %.1e) within_1e-2 %.5f within_1e-4 %.5f (bound %.2f)" % (m["rel_l2"], rel_l2, m["frac_within_1e-2"], m["frac_within_1e-4"], within_1e4))
    assert np.isfinite(g["accum"]).all()
    assert m["rel_l2"] <= rel_l2, m
    assert m["frac_within_1e-2"] >= within_1e2, m
    assert m["frac_within_1e-4"] >= within_1e4, m
    assert m["alpha_max_abs"] <= alpha_tol, m
    assert (o["selection"] == g["selection"]).mean() >= 0.9999
    assert np.abs(o["depth"] - g["depth"]).max() <= depth_tol
    for k in COUNTERS:
        a, b = o["stats"][k], g["stats"][k]
        assert abs(a - b) <= max(2, counter_rel * a), (k, a, b)


SIDE_STREAM = {"MI_PT_OVERLAP_MIN_TRIS": 0}


def test_opaque_scene_both_acceleration_structures(built, assets):
    """Case 1 -- MODE 0: Box.glb under the sky and the default directional light, 64x48, depth 4, 4 frames; 1 and 4 in flight, 8-wide BVH and BVH2."""
    s = pu.Setup(os.path.join(assets, "Box.glb"), 64, 48, max_depth=4)
    oracle = pu.render_oracle(s, 4)
    for bvh in (0, 1):
        for in_flight in (1, 4):
            on = _render(s, 4, 1, SIDE_STREAM, bvh=bvh, in_flight=in_flight)
            _same(on, _render(s, 4, 0, SIDE_STREAM, bvh=bvh, in_flight=in_flight), (bvh, in_flight))
            _check(oracle, on, ("box", bvh, in_flight), rel_l2=6e-3)  # (test_box_sky: the sun disc is in play)
            # ... and the instantiations without the ray counters (<WIDE, 0, false>: what a caller who does not ask for statistics runs): same bytes
            plain = _render(s, 4, 1, SIDE_STREAM, bvh=bvh, in_flight=in_flight, collect_counters=False)
            _same_images(plain, _render(s, 4, 0, SIDE_STREAM, bvh=bvh, in_flight=in_flight, collect_counters=False), (bvh, in_flight, "no counters"))
            _same_images(plain, on, (bvh, in_flight, "counters or not"))


def test_alpha_tested_scene(built, tmp_path):
    """Case 2 -- MODE 1: the scene of test_atrium_class_alpha_lights at its resolution (alpha rounds; rays that end while their alpha tests are pending), 3 frames; 1
    and 3 in flight."""
    path = scenegen.scene_atrium_class(str(tmp_path / "atrium.glb"), seed=5, detail=0.12, tex_size=64)
    s = pu.Setup(path, 160, 96, max_depth=8)
    oracle = pu.render_oracle(s, 3)
    for in_flight in (1, 3):
        on = _render(s, 3, 1, SIDE_STREAM, in_flight=in_flight)
        _same(on, _render(s, 3, 0, SIDE_STREAM, in_flight=in_flight), in_flight)
        _check(oracle, on, ("atrium", in_flight), rel_l2=1e-3)
        # ... and <true, 1, false>, the instantiation that asks for the contribution when the ray starts (the counting one takes it the same way but is
        # compiled on its own): same bytes
        plain = _render(s, 3, 1, SIDE_STREAM, in_flight=in_flight, collect_counters=False)
        _same_images(plain, _render(s, 3, 0, SIDE_STREAM, in_flight=in_flight, collect_counters=False), (in_flight, "no counters"))
        _same_images(plain, on, (in_flight, "counters or not"))


def test_batch_of_64_and_single_frames_on_one_stream(built, assets):
    """Case 3 -- case 1 at 32x16, depth 3: 64 frames in flight in one call (pixel-major slots: a wave holds 64 samples of one pixel), then the same 64 frames one by
    one; both on the single-stream schedule (the scene is below MI_PT_OVERLAP_MIN_TRIS)."""
    s = pu.Setup(os.path.join(assets, "Box.glb"), 32, 16, max_depth=3)
    oracle = pu.render_oracle(s, 64)
    for in_flight in (64, 1):
        on = _render(s, 64, 1, in_flight=in_flight)
        _same(on, _render(s, 64, 0, in_flight=in_flight), in_flight)
        _check(oracle, on, ("box 64 frames", in_flight), rel_l2=6e-3)


def _plane(catcher, distance=-0.62):
    def edit(fi):
        fi.flags |= capi.MI_SCENE_USE_INFINITE_PLANE | (capi.MI_SCENE_INFINITE_PLANE_SHADOW_CATCHER if catcher else 0)
        fi.infinitePlaneDistance = distance
        fi.infinitePlaneBaseColor[:] = [0.7, 0.6, 0.5]
        fi.infinitePlaneMetallic, fi.infinitePlaneRoughness, fi.shadowCatcherDarkenAmount = 0.1, 0.45, 0.35
    return edit


def test_catcher_probes_and_deposits_in_one_frame(built, assets):
    """Case 4 -- the frames of test_shadow_catcher_plane (Box.glb 192x144, depth 4, 8 frames, under the HDR map and under the sky): the probes of the plane go through
    k_shadow_resolve, the shadow rays of the box are deposited by the walk, in the same launch pair; frame by frame on the 8-wide BVH and 4 in flight on the BVH2."""
    hdr = os.path.join(assets, "std_env.hdr")
    for kw in (dict(hdr_path=hdr), dict()):
        s = pu.Setup(os.path.join(assets, "Box.glb"), 192, 144, max_depth=4, frame_info_edit=_plane(True), **kw)
        on = _render(s, 8, 1)
        _same(on, _render(s, 8, 0), sorted(kw))
        _check(pu.render_oracle(s, 8), on, ("catcher", sorted(kw)), rel_l2=1e-2 if not kw else 1e-3)
        on4 = _render(s, 8, 1, in_flight=4, bvh=1)
        _same(on4, _render(s, 8, 0, in_flight=4, bvh=1), (sorted(kw), "4 in flight, BVH2"))
        assert on["accum"].tobytes() == on4["accum"].tobytes()


def test_path_state_kept_by_slot(built, assets):
    """Case 5 -- case 1 with MI_PT_STATE_BY_SLOT: every ray's target is PathSoA::radiance[slot], not only that of paths which ended at the bounce."""
    s = pu.Setup(os.path.join(assets, "Box.glb"), 64, 48, max_depth=4)
    oracle = pu.render_oracle(s, 4)
    env = dict(SIDE_STREAM, MI_PT_STATE_BY_SLOT=1)
    for bvh in (0, 1):
        for in_flight in (1, 4):
            on = _render(s, 4, 1, env, bvh=bvh, in_flight=in_flight)
            _same(on, _render(s, 4, 0, env, bvh=bvh, in_flight=in_flight), (bvh, in_flight))
            _check(oracle, on, ("box by slot", bvh, in_flight), rel_l2=6e-3)


def test_empty_acceleration_structure(built, tmp_path):
    """Case 6 -- a scene without geometry over the infinite plane: every shadow ray starts on the plane and takes the walk's BVH_EMPTY shortcut, as a plain ray (the
    plane as a surface: deposited by the walk) and as a catcher probe (through the resolve kernel)."""
    b = scenegen.GlbBuilder()
    b.camera_node((0, 0.4, 3), (0, 0, 0))
    path = b.save(str(tmp_path / "nothing.glb"))
    for catcher in (False, True):
        s = pu.Setup(path, 64, 48, max_depth=4, frame_info_edit=_plane(catcher))
        oracle = pu.render_oracle(s, 4)
        for bvh in (0, 1):
            on = _render(s, 4, 1, bvh=bvh, in_flight=2)
            _same(on, _render(s, 4, 0, bvh=bvh, in_flight=2), (catcher, bvh))
            _check(oracle, on, ("plane alone", catcher, bvh), rel_l2=1e-2 if catcher else 6e-3)  # (test_shadow_catcher_plane / test_infinite_plane under the sky)


# ---- the instruction ------------------------------------------------------------------------------------------------------------------------------------------------
def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


MAXF, MINN = np.float32(3.4028235e38), np.float32(1.17549435e-38)
KAT_ROWS = [  # (record, term)
    # ordinary values
    (1.0, 2.0), (0.1, 0.2), (0.75, -0.5), (123456.789, 0.001), (-3.5, 1.25), (1e10, 1.0), (1e-10, 1e-12), (2.5e-3, 7.0e4), (-1e20, 1e20), (6.0, -6.0), (-6.0, 6.0),
    # zeros of both signs
    (0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 1.5), (-0.0, 1.5), (1.5, -0.0),
    # sums that round: ties to even both ways, just above and just below the tie, both signs
    (1.0, 2.0 ** -24), (1.0 + 2.0 ** -23, 2.0 ** -24), (1.0, 2.0 ** -24 + 2.0 ** -40), (1.0, 2.0 ** -24 - 2.0 ** -47), (-1.0, -(2.0 ** -24)), (-1.0 - 2.0 ** -23, -(2.0 ** -24)),
    (-1.0, -(2.0 ** -24 + 2.0 ** -40)), (1.0, -(2.0 ** -25)), (1.0, -(2.0 ** -25 + 2.0 ** -45)), (1.0 - 2.0 ** -24, -(2.0 ** -25)), (16777216.0, 1.0), (16777216.0, 3.0), (16777218.0, 1.0),
    (1.0, 1e-30), (-1.0, 1e-30),
    # overflow
    (3.0e38, 3.0e38), (3.0e38, 1.0e38), (3.0e38, 4.0e37), (-3.0e38, -3.0e38), (MAXF, 2.0 ** 103), (MAXF, 2.0 ** 102), (-MAXF, -(2.0 ** 103)), (MAXF, MAXF), (MAXF, -MAXF),
    # infinities
    (np.inf, 1.0), (1.0, np.inf), (np.inf, np.inf), (-np.inf, -1.0), (1.0, -np.inf), (-np.inf, MAXF), (np.inf, -np.inf),
    # denormal operands and results (printed, not asserted)
    (0.0, 1e-40), (1e-40, 0.0), (1e-40, 1e-40), (1.0, 1e-40), (1e-40, 1.0), (MINN, -1e-40), (MINN, 1e-40), (_f(0x00400000), _f(0x00400000)), (_f(1), _f(1)), (-0.0, -1e-40),
    (1.5 * float(MINN), -float(MINN)), (float(MINN), -1.5 * float(MINN)), (3.0 * float(MINN), -2.5 * float(MINN)), (_f(0x007fffff), _f(1)), (-1e-40, 1e-40), (MINN, -MINN),
]


def test_the_memory_side_add_is_the_float32_add():
    assert len(KAT_ROWS) <= 192
    rec = np.full(192, 1.0, np.float32)
    term = np.full(192, 0.5, np.float32)
    for i, (a, b) in enumerate(KAT_ROWS):
        rec[i], term[i] = np.float32(a), np.float32(b)
    with np.errstate(all="ignore"):
        want = (rec + term).astype(np.float32)
    rad = np.zeros((64, 4), np.float32)
    rad[:, :3] = rec.reshape(64, 3)
    w = (0x7fc01234 + np.arange(64)).astype(np.uint32)  # (.w: a payload nobody may touch)
    rad[:, 3] = w.view(np.float32)
    c = np.ascontiguousarray(term.reshape(64, 3))
    fn = kat.lib().kat_atomic_deposit
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    err = fn(rad.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p))
    assert err == 0, "kat_atomic_deposit: hipError_t %d" % err
    assert (rad[:, 3].view(np.uint32) == w).all()
    got = np.ascontiguousarray(rad[:, :3]).reshape(192)

    def plain(x):  # normal, zero or infinite
        return (x == 0) | np.isinf(x) | (np.isfinite(x) & (np.abs(x) >= MINN))

    asserted = plain(rec) & plain(term) & plain(want)
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    for i in np.nonzero(~asserted)[0]:
        print("KAT row %3d  %-15r (0x%08x) + %-15r (0x%08x): device 0x%08x %-15r numpy 0x%08x %-15r %s" % (i, rec[i], rec.view(np.uint32)[i], term[i], term.view(np.uint32)[i], gb[i], got[i], wb[i], want[i],
                                                                                                        "same" if gb[i] == wb[i] or (np.isnan(got[i]) and np.isnan(want[i])) else "DIFFERENT"))
    assert asserted.sum() >= 192 - 24
    bad = np.nonzero(asserted & (gb != wb))[0]
    assert len(bad) == 0, [(int(i), float(rec[i]), float(term[i]), hex(int(gb[i])), hex(int(wb[i]))) for i in bad]
