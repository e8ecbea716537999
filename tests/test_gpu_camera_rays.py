"""Caller-supplied camera rays on the GPU (mi_pt_set_camera_rays, mi_pt_set_camera_rays_device, mi_pt_make_camera_rays and its device form;
csrc/device/camera_rays.hip, pt_camera_rays.h).

1. binding (unit=True) what make_camera_rays wrote reproduces the built-in camera's single-sample frames byte for byte -- accumulator, guides,
   depth, first hit, selection -- with a thin lens and orthographic, on both trees, at 1, 3 and 64 frames in flight, under a tile partition;
2. unbinding restores the fused packet kernel and the bytes of a never-bound instance;
3. a path follows its RAY, not its pixel: permuted rays give the permuted first-hit, selection and environment-only images;
4. the selection image is renderNode + 1 of query_rays("closest") over the bound set;
5. dead rays (a fisheye mask, NaN / inf / zero directions, a whole wave, a whole set) start no path and poison nothing;
6. K sets repeat with period K; multi-sample frames render and repeat;
7. directions are normalised once unless unit=True;
8. state and argument errors leave the binding unchanged; memory.
The torch half (device forms) runs in tests/camera_rays_device_child.py.

The image is 72 x 40: partial 8 x 8 micro-tiles (40 = 5 x 8, 72 = 9 x 8 with 64-pixel tiles cut at 8 and 40) and partial tiles.  Byte equality
throughout: the feature adds no arithmetic to a path, it only changes where its first ray comes from.  Two images stay out of comparison 1: the
first-hit triangle image exists only under mi_pt_set_temporal + vertex motion, which bound rays refuse; and the selection image of a bound set is
that set's closest query (4), where the built-in camera's is the un-jittered, lens-free ray through the pixel centre."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as pu
import query_util as qu
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 72, 40
DEPTH = 4
IN_FLIGHT = (1, 3, 64)
SCENES = ("mixed_alpha_glass", "animated")
F32 = np.float32


@contextlib.contextmanager
def _environment(values):
    """MI_PT_* switches are read once, in mi_pt_create: set for the instances created inside, restored afterwards."""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_camera_rays")
    return {name: qu.make_scene(name, d) for name in SCENES}


@pytest.fixture(scope="module")
def hdr_pixels():
    rng = np.random.default_rng(3)
    return np.ascontiguousarray(rng.uniform(0.05, 2.0, (16, 32, 3)), F32)


def _setup(path, kind="lens", hdr=None, spp=1):
    scene = ptmod.Scene(path)
    cam = scene.camera(0)
    scene.close()
    if kind == "ortho":
        cam.orthographic, cam.xmag, cam.ymag = 1, 4.0, 3.0

    def edit(p):
        if kind == "lens":
            p.aperture = 0.05
    return pu.Setup(path, W, H, max_depth=DEPTH, spp_per_frame=spp, camera=cam, params_edit=edit, hdr_pixels=hdr)


def _tracer(st, no_packet=False, **kw):
    with _environment({"MI_PT_NO_PACKET": "1"} if no_packet else {}):
        tr = ptmod.PathTracer(st.scene, **kw)
    if st.hdr is not None:
        tr.set_environment(st.hdr)
    tr.resize(W, H)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    return tr


def _params(st, start, first, guides=True):
    p = st.frame_params(start, start * st.params.numSamples)
    p.flags = (capi.MI_PT_FIRST_FRAME if first else 0) | (capi.MI_PT_USE_OPTIX_DENOISER if guides else 0)
    return p


def _images(tr):
    albedo, normal = tr.read_guides()
    return {"accum": tr.read_accum(), "albedo": albedo, "normal": normal, "depth": tr.read_depth(), "first_hit": tr.read_first_hit(),
            "selection": tr.read_selection()}


def _render(tr, st, n, batches=1, guides=True):
    """`batches` batches of n frames from frame 0 on, the first one a first-frame batch."""
    for b in range(batches):
        tr.render_frames(_params(st, b * n, b == 0, guides), n)
    return _images(tr)


def _same(a, b, what, mask=None, skip=()):
    for k in a:
        if k in skip:
            continue
        x, y = a[k].view(np.uint32), b[k].view(np.uint32)
        if mask is not None:
            x, y = x[mask], y[mask]
        assert (x == y).all(), (what, k, int((x != y).sum()))


def _rel_l2(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b) ** 2).sum() / max((a.astype(np.float64) ** 2).sum(), 1e-30)))


def _centre_camera(scene):
    lo, hi = scene.bounds()
    c = (np.asarray(lo, np.float64) + np.asarray(hi, np.float64)) / 2
    cam = scene.camera(0)
    cam.eye[:] = [float(v) for v in c]
    cam.center[:] = [float(c[0]), float(c[1]), float(c[2] - 1.0)]
    cam.up[:] = [0.0, 1.0, 0.0]
    cam.orthographic = 0
    return cam


# ---- 1. export == built-in ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", [0, 1])
@pytest.mark.parametrize("kind", ["lens", "ortho"])
@pytest.mark.parametrize("scene", SCENES)
def test_exported_rays_reproduce_the_builtin_camera(paths, scene, kind, bvh):
    st = _setup(paths[scene], kind)
    tr = _tracer(st, no_packet=True, bvh=bvh)
    for n in IN_FLIGHT:
        tr.set_camera_rays(None)
        want = _render(tr, st, n, batches=2)
        rays = tr.make_camera_rays(_params(st, 0, True), 2 * n)
        assert rays.shape == (2 * n, H, W, 8) and np.isfinite(rays[..., :7]).all()
        assert (rays[..., 3] == 0).all() and (rays[..., 7] == np.finfo(F32).max).all()
        assert np.abs(np.linalg.norm(rays[..., 4:7].astype(np.float64), axis=-1) - 1).max() < 1e-6
        if n > 1:
            assert (rays[0] != rays[1]).any()  # (jittered sets)
        tr.set_camera_rays(rays, unit=True)
        got = _render(tr, st, n, batches=2)
        # (not the selection image: the built-in camera's comes from the un-jittered pixel centre, a bound set's from the set itself -- test 4)
        _same(want, got, (scene, kind, bvh, n), skip=("selection",))
        assert (want["selection"] != 0).sum() > 100 and np.isfinite(want["accum"]).all()
    tr.close()


def test_exported_rays_under_a_tile_partition(paths):
    st = _setup(paths["animated"], "lens")
    tr = _tracer(st, no_packet=True)
    tr.set_tile_partition(1, 2, 32)
    want = _render(tr, st, 3, batches=2)
    rays = tr.make_camera_rays(_params(st, 0, True), 6)
    whole = _tracer(st, no_packet=True)
    assert whole.make_camera_rays(_params(st, 0, True), 6).tobytes() == rays.tobytes()  # every pixel, whatever the partition
    whole.close()
    tr.set_camera_rays(rays, unit=True)
    got = _render(tr, st, 3, batches=2)
    _same(want, got, "partition", skip=("selection",))
    ys, xs = np.mgrid[0:H, 0:W]
    other = ((ys // 32) * ((W + 31) // 32) + xs // 32) % 2 != 1
    assert other.any() and (~other).any()
    assert (got["accum"][other] == 0).all() and (got["selection"][other] == 0).all() and (got["accum"][~other] != 0).any()
    tr.close()


def test_packet_instance_for_information(paths):
    """Not an equality: the fused packet kernel walks the same camera rays but finishes its misses elsewhere.  Prints the rel-L2 of the bound
    frames against a default instance; asserts only that they are finite."""
    st = _setup(paths["animated"], "lens")
    a, b = _tracer(st), _tracer(st, no_packet=True)
    want = _render(a, st, 3, batches=2)
    b.set_camera_rays(b.make_camera_rays(_params(st, 0, True), 6), unit=True)
    got = _render(b, st, 3, batches=2)
    r = _rel_l2(want["accum"], got["accum"])
    print("camera rays against the packet instance: rel-L2 = %.3e" % r)
    assert np.isfinite(got["accum"]).all() and np.isfinite(r)
    a.close()
    b.close()


# ---- 2. unbind --------------------------------------------------------------------------------------------------------------------------------------
def test_unbinding_restores_the_packet_kernel(paths):
    st = _setup(paths["mixed_alpha_glass"], "lens")
    tr, fresh = _tracer(st), _tracer(st)
    tr.enable_timing(True)
    tr.set_camera_rays(tr.make_camera_rays(_params(st, 0, True), 3), unit=True)
    t0 = tr.frame_timing()
    _render(tr, st, 3)
    t1 = tr.frame_timing()
    assert t1["tracePrimaryLaunches"] == t0["tracePrimaryLaunches"] and t1["generateMs"] > t0["generateMs"], (t0, t1)
    tr.set_camera_rays(None)
    got = _render(tr, st, 3)
    t2 = tr.frame_timing()
    assert t2["tracePrimaryLaunches"] > t1["tracePrimaryLaunches"], (t1, t2)
    _same(_render(fresh, st, 3), got, "unbind")
    tr.close()
    fresh.close()


# ---- 3. ray, not pixel ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", [0, 1])
def test_a_path_follows_its_ray_not_its_pixel(paths, hdr_pixels, bvh):
    st = _setup(paths["animated"], "pinhole", hdr=hdr_pixels)
    rays, angle = ptmod.camera_rays(_centre_camera(st.scene), W, H, "equirect")
    st.params.pixelAngle = angle
    perm = np.random.default_rng(11).permutation(W * H)
    moved = rays.reshape(-1, 8)[perm].reshape(1, H, W, 8)
    tr = _tracer(st, bvh=bvh)
    tr.set_camera_rays(rays, unit=True)
    a = _render(tr, st, 1)
    tr.set_camera_rays(moved, unit=True)
    b = _render(tr, st, 1)
    tr.close()

    def permuted(img):
        return img.reshape(W * H, -1)[perm].reshape(img.shape)
    assert (permuted(a["selection"]) == b["selection"]).all()
    assert (permuted(a["first_hit"]).view(np.uint32) == b["first_hit"].view(np.uint32)).all()
    sky = a["first_hit"].view(np.uint32)[..., 3] == 0  # the camera ray left the scene: the path ended at bounce 0 with the environment
    assert 100 < sky.sum() < W * H - 100, int(sky.sum())
    sky_moved = permuted(sky)
    assert (permuted(a["accum"]).view(np.uint32)[sky_moved] == b["accum"].view(np.uint32)[sky_moved]).all()
    assert (a["accum"][sky][:, :3] > 0).any() and (a["accum"][sky][:, 3] == 0).all()


# ---- 4. selection = query ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", [0, 1])
@pytest.mark.parametrize("scene", SCENES)
def test_selection_is_the_closest_query_of_the_bound_set(paths, scene, bvh):
    st = _setup(paths[scene], "lens")
    tr = _tracer(st, bvh=bvh)
    equirect, _ = ptmod.camera_rays(_centre_camera(st.scene), W, H, "equirect", jitter=[(0.5, 0.5), (0.25, 0.75)])
    exported = tr.make_camera_rays(_params(st, 0, True), 2)
    for rays in (equirect, exported):
        for start in (0, 1):  # the set of the batch's first frame
            tr.set_camera_rays(rays, unit=True)
            tr.render_frames(_params(st, start, True), 2)
            hits = tr.query_rays(rays[start % 2].reshape(-1, 8))
            assert (tr.read_selection().reshape(-1).astype(np.int64) == hits["renderNode"].astype(np.int64) + 1).all()
            assert (hits["renderNode"] >= 0).sum() > 100
    tr.close()


# ---- 5. dead rays -----------------------------------------------------------------------------------------------------------------------------------
def _dead_sets(scene):
    fish, angle = ptmod.camera_rays(scene.camera(0), W, H, "fisheye", fov=150.0, jitter=[(0.5, 0.5), (0.3, 0.6), (0.7, 0.4)])
    masked = (fish[..., 4:7] == 0).all(-1)  # (per set: the jitter moves the circle's rim by a fraction of a pixel)
    outside, rim = masked.all(0), masked.any(0) & ~masked.all(0)
    assert outside[:8, :8].all() and not masked[:, 16:24, 32:40].any()  # whole waves outside the circle, whole waves inside
    valid = fish.copy()
    dead = fish.copy()
    nan, inf = F32(np.nan), F32(np.inf)
    dead[0, 20, 30, 4] = nan        # direction x
    dead[0, 20, 31, 6] = -inf       # direction z
    dead[0, 21, 33, 0] = nan        # origin x
    dead[0, 21, 35, 2] = inf        # origin z
    dead[0, 19, 37, 4:7] = 0        # zero direction
    dead[1, 22, 36, 5] = nan        # ... in another set
    dead[2, 16:24, 40:48, 4:7] = 0  # a whole wave among living ones
    killed = np.zeros((H, W), bool)
    for y, x in ((20, 30), (20, 31), (21, 33), (21, 35), (19, 37), (22, 36)):
        killed[y, x] = True
    killed[16:24, 40:48] = True
    assert not (killed & (outside | rim)).any()
    return valid, dead, outside, killed | rim, angle


@pytest.mark.parametrize("bvh", [0, 1])
def test_dead_rays_start_no_path(paths, hdr_pixels, bvh):
    st = _setup(paths["mixed_alpha_glass"], "pinhole", hdr=hdr_pixels)
    valid, dead, outside, killed, angle = _dead_sets(st.scene)
    st.params.pixelAngle = angle
    tr = _tracer(st, bvh=bvh)
    tr.set_camera_rays(valid)
    want = _render(tr, st, 3)
    tr.set_camera_rays(dead)
    got = _render(tr, st, 3)
    assert all(np.isfinite(v).all() for k, v in got.items() if k != "selection")
    # never alive: everything a first frame writes for the pixel is the empty value
    assert (got["accum"][outside] == 0).all() and (got["selection"][outside] == 0).all() and (got["depth"][outside] == 1).all()
    assert (got["first_hit"].view(np.uint32)[outside][:, 3] == 0).all()
    assert (got["albedo"][outside] == 0).all() and (got["normal"][outside] == 0).all()
    # alive in every set: the bytes of the run in which the others were alive too
    _same(want, got, "live pixels", mask=~(outside | killed))
    assert (want["accum"][~outside][:, :3] > 0).any()
    # dead in some frame (killed above, or on the circle's rim): that frame folded radiance 0, alpha 0 into the running mean
    assert (got["accum"].view(np.uint32)[killed] != want["accum"].view(np.uint32)[killed]).any()
    # a set that is entirely dead, between two living ones; then nothing but dead rays
    sets = np.stack([valid[0], np.zeros_like(valid[0]), valid[0]])
    tr.set_camera_rays(sets)
    mixed = _render(tr, st, 3)
    assert all(np.isfinite(v).all() for k, v in mixed.items() if k != "selection")
    solid = (mixed["selection"] != 0) & (want["depth"] < 1)
    tr.set_camera_rays(np.full((1, H, W, 8), np.nan, F32))
    none = _render(tr, st, 3)
    assert (none["accum"] == 0).all() and (none["selection"] == 0).all() and (none["depth"] == 1).all() and (none["albedo"] == 0).all()
    assert (none["first_hit"] == 0).all()
    assert solid.sum() > 50
    tr.close()


def test_an_entirely_dead_set_is_one_empty_frame(paths):
    """Two frames, one of them over a set that is entirely dead: the running mean is (sample + 0) / 2, exactly half the living frame's sample in
    every channel -- whichever of the two frames is the dead one."""
    st = _setup(paths["animated"], "pinhole")
    rays = ptmod.camera_rays(st.scene.camera(0), W, H, "perspective")[0]
    none = np.zeros_like(rays[0])
    tr = _tracer(st)
    for sets, alive in (([rays[0], none], 0), ([none, rays[0]], 1)):
        tr.set_camera_rays(np.stack(sets), unit=True)
        tr.render_frames(_params(st, alive, True), 1)  # the living frame alone: frame `alive` takes set `alive`
        one = _images(tr)
        assert (one["accum"][..., 3] == 1).sum() > 100 and np.isfinite(one["accum"]).all()
        two = _render(tr, st, 2)
        assert (two["accum"].view(np.uint32) == (one["accum"] * F32(0.5)).view(np.uint32)).all()
        if alive == 1:  # the first frame was the dead one: nothing was hit, whatever the second frame saw
            assert (two["selection"] == 0).all() and (two["depth"] == 1).all() and (two["first_hit"] == 0).all()
        else:
            assert (two["selection"] == one["selection"]).all() and (two["depth"] == one["depth"]).all()
    tr.close()


# ---- 6. sets and samples ------------------------------------------------------------------------------------------------------------------------
def test_sets_repeat_and_multi_sample_frames(paths):
    st = _setup(paths["mixed_alpha_glass"], "pinhole")
    rng = np.random.default_rng(5)
    two = ptmod.camera_rays(st.scene.camera(0), W, H, "perspective", jitter=rng.uniform(0, 1, (2, 2)))[0]
    tr = _tracer(st)
    tr.set_camera_rays(two, unit=True)
    a = _render(tr, st, 3, batches=2)
    tr.set_camera_rays(np.concatenate([two, two, two]), unit=True)
    b = _render(tr, st, 3, batches=2)
    _same(a, b, "K = 2 against K = 6")
    tr.close()
    st2 = _setup(paths["mixed_alpha_glass"], "pinhole", spp=2)
    tr = _tracer(st2)
    tr.set_camera_rays(two, unit=True)
    c = _render(tr, st2, 3, batches=2)
    d = _render(tr, st2, 3, batches=2)
    _same(c, d, "two samples per frame, twice")
    assert np.isfinite(c["accum"]).all() and (c["accum"][..., :3] > 0).any()
    assert (c["accum"] != a["accum"]).any()
    tr.close()


# ---- 7. normalisation -----------------------------------------------------------------------------------------------------------------------------
def _normalize_is_identity(d):
    """Pixels whose float32 direction normalises to itself: 1 / sqrt(dot) is exactly 1 iff the float32 dot is 1 or 1 + 2^-23 (whose square root lies
    just below 1 + 2^-24 and rounds to 1; that of 1 - 2^-24 rounds to itself).  The compiler may contract the dot product's multiply-adds or not:
    all four ways must agree."""
    x, y, z = (d[..., i].astype(np.float64) for i in range(3))
    r32 = lambda v: v.astype(F32).astype(np.float64)  # noqa: E731
    ok = np.ones(d.shape[:-1], bool)
    good = (np.float64(1), np.float64(1) + 2.0 ** -23)
    for fma_y in (False, True):
        for fma_z in (False, True):
            s = r32(x * x)
            s = r32(y * y + s) if fma_y else r32(r32(y * y) + s)
            s = r32(z * z + s) if fma_z else r32(r32(z * z) + s)
            ok &= np.isin(s, good)
    return ok


def test_directions_are_normalised_once_unless_unit(paths):
    st = _setup(paths["animated"], "pinhole")
    rays = ptmod.camera_rays(st.scene.camera(0), W, H, "perspective")[0]
    tr = _tracer(st)
    tr.set_camera_rays(rays, unit=True)
    unit = _render(tr, st, 3)
    tr.set_camera_rays(rays)
    plain = _render(tr, st, 3)
    same = _normalize_is_identity(rays[0, ..., 4:7])
    assert same.sum() > W * H // 4, int(same.sum())
    _same(unit, plain, "normalize is the identity", mask=same)
    scaled = rays.copy()
    scaled[..., 4:7] *= F32(3.7)
    tr.set_camera_rays(scaled)
    long = _render(tr, st, 3)
    assert (long["selection"] == unit["selection"]).all()
    assert (long["first_hit"].view(np.uint32)[..., 3] == unit["first_hit"].view(np.uint32)[..., 3]).all()
    assert np.isfinite(long["accum"]).all() and _rel_l2(unit["accum"], long["accum"]) < 0.5
    tiny = rays.copy()
    tiny[..., 4:7] *= F32(1e-42)  # denormal directions are directions
    tr.set_camera_rays(tiny)
    small = _render(tr, st, 3)
    # (the selection image walks the ray as given, like the query it equals: at this scale every hit lies beyond the far bound)
    assert np.isfinite(small["accum"]).all() and (small["first_hit"].view(np.uint32)[..., 3] == unit["first_hit"].view(np.uint32)[..., 3]).mean() > 0.99
    tr.close()


# ---- 8. state and arguments -------------------------------------------------------------------------------------------------------------------------
def test_state_argument_errors_and_memory(paths):
    st = _setup(paths["animated"], "pinhole")
    with _environment({}):
        tr = ptmod.PathTracer(st.scene)
    L, p = tr._l, tr._p
    rays = ptmod.camera_rays(st.scene.camera(0), W, H, "perspective", jitter=[(0.5, 0.5), (0.2, 0.8)])[0]
    ptr = rays.ctypes.data_as(capi.P(capi.MiPtRay))
    ARG, STATE = -1, -4
    assert L.mi_pt_set_camera_rays(p, ptr, 2, 0) == STATE  # before mi_pt_resize
    assert L.mi_pt_make_camera_rays(p, st.params, 2, ptr) == STATE
    tr.resize(W, H)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    _render(tr, st, 2)  # (the path arrays and the guide records of a 2-frame batch exist from here on)
    base = tr.memory()
    tr.set_camera_rays(rays, unit=True)
    m = tr.memory()
    assert m["rendererBytes"] - base["rendererBytes"] == 2 * W * H * 32 and m["sceneBytes"] == base["sceneBytes"], (base, m)
    bound = _render(tr, st, 2)
    assert tr.memory() == m or tr.memory()["rendererBytes"] == m["rendererBytes"]
    tr.set_camera_rays(None)
    assert tr.memory()["rendererBytes"] == base["rendererBytes"]  # given back on unbind
    tr.set_camera_rays(rays, unit=True)
    for args in ((ptr, 0, 0), (ptr, -1, 0), (None, 1, 0), (ptr, 2, 2), (ptr, 2, 0x80000000)):
        assert L.mi_pt_set_camera_rays(p, *args) == ARG, args
    assert L.mi_pt_set_camera_rays_device(p, 16 + 4, 2, 0) == ARG  # not 16-byte aligned
    assert L.mi_pt_make_camera_rays(p, None, 2, ptr) == ARG and L.mi_pt_make_camera_rays(p, st.params, 2, None) == ARG
    assert L.mi_pt_make_camera_rays(p, st.params, 0, ptr) == ARG
    assert L.mi_pt_make_camera_rays_device(p, st.params, 1, 16 + 8, None) == ARG
    with pytest.raises(ptmod.MiError):
        tr.set_temporal(True)  # the motion image assumes the projective camera
    assert tr.memory()["rendererBytes"] == m["rendererBytes"]
    _same(bound, _render(tr, st, 2), "the binding survived every refusal")
    # resize: the render calls refuse until the caller binds or unbinds again
    tr.resize(W + 8, H)
    prm = _params(st, 0, True)
    assert L.mi_pt_render_frames(p, prm, 2, None) == STATE and L.mi_pt_render_frame(p, prm, None) == STATE
    tr.set_frame_queue(4)
    assert L.mi_pt_render_frame(p, prm, None) == STATE
    tr.set_frame_queue(1)
    tr.resize(W, H)  # (the size they were bound at)
    tr.set_frame_info(st.frame_info)
    _same(bound, _render(tr, st, 2), "back at the bound size")
    tr.resize(W + 8, H)
    tr.set_camera_rays(None)
    assert tr.memory()["rendererBytes"] < m["rendererBytes"]
    tr.render_frames(prm, 2)
    tr.resize(W, H)
    tr.set_frame_info(st.frame_info)
    tr.set_camera_rays(rays, unit=True)
    _same(bound, _render(tr, st, 2), "bound again")
    # temporal on: binding refuses; the binding in force is the one before
    tr.set_camera_rays(None)
    unbound = _render(tr, st, 2)
    tr.set_temporal(True)
    assert L.mi_pt_set_camera_rays(p, ptr, 2, 0) == STATE
    tr.set_temporal(False)
    _same(unbound, _render(tr, st, 2), "still the built-in camera")
    assert (unbound["accum"] != bound["accum"]).any()
    # a bind between queued frames flushes them: the frames before it used the binding of their time
    tr.set_frame_queue(4)
    tr.render_frame(_params(st, 0, True))
    tr.render_frame(_params(st, 1, False))
    tr.set_camera_rays(rays, unit=True)
    tr.set_frame_queue(1)
    _same({"accum": unbound["accum"]}, {"accum": tr.read_accum()}, "queued frames were flushed before the bind")
    tr.close()


def test_device_forms_with_torch_tensors(tmp_path):
    """In a process of its own (tests/camera_rays_device_child.py), like the device form of the queries: torch is loaded first there."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "camera_rays_device_child.py"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "CAMERA_RAYS_DEVICE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
