"""The device tonemapper (replaces GltfRenderer::tonemap -> nvshaders::Tonemapper, reference src/renderer.cpp:992-1056,
method set src/renderer.cpp:173-179) against the PUBLISHED form of each operator written in numpy float64: Hejl / Burgess-Dawson
filmic, Hable "Uncharted 2" (W = 11.2, exposure bias 2), S. Hill's ACES fit, B. Wrensch's minimal AgX, Khronos PBR Neutral, IEC
61966-2-1 sRGB.  8-bit outputs may differ by one code where the float32 device arithmetic rounds the other way."""
import os

import numpy as np
import pytest

import parity_util as pu
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

pytestmark = pytest.mark.gpu


def _srgb(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 0.0031308, 1.055 * np.power(np.maximum(x, 1e-30), 1 / 2.4) - 0.055, 12.92 * x)


def _filmic(c):
    t = np.maximum(0.0, c - 0.004)
    return (t * (6.2 * t + 0.5)) / (t * (6.2 * t + 1.7) + 0.06)


def _hable(x):
    a, b, c, d, e, f = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30
    return ((x * (a * x + c * b) + d * e) / (x * (a * x + b) + d * f)) - e / f


def _uncharted(c):
    return _srgb(_hable(c * 2.0) / _hable(11.2))


def _aces(c):
    m_in = np.array([[0.59719, 0.35458, 0.04823], [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.83777]])
    m_out = np.array([[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605], [-0.00327, -0.07276, 1.07602]])
    v = c @ m_in.T
    v = (v * (v + 0.0245786) - 0.000090537) / (v * (0.983729 * v + 0.4329510) + 0.238081)
    return _srgb(v @ m_out.T)


def _agx(c):
    # column-major GLSL mat3 constants of the published minimal AgX, written here as row-major numpy matrices (transposed)
    inset = np.array([[0.842479062253094, 0.0784335999999992, 0.0792237451477643], [0.0423282422610123, 0.878468636469772, 0.0791661274605434],
                      [0.0423756549057051, 0.0784336, 0.879142973793104]])
    outset = np.array([[1.19687900512017, -0.0980208811401368, -0.0990297440797205], [-0.0528968517574562, 1.15190312990417, -0.0989611768448433],
                       [-0.0529716355144438, -0.0980434501171241, 1.15107367264116]])
    lo, hi = -12.47393, 4.026069
    v = c @ inset.T
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (np.clip(np.where(v > 0, np.log2(np.maximum(v, 1e-300)), lo), lo, hi) - lo) / (hi - lo)
    x2, x4 = x * x, x * x * x * x
    v = 15.5 * x4 * x2 - 40.14 * x4 * x + 31.96 * x4 - 6.868 * x2 * x + 0.4298 * x2 + 0.1191 * x - 0.00232
    return v @ outset.T


def _khronos(c):
    start, desat = 0.8 - 0.04, 0.15
    x = c.min(-1, keepdims=True)
    c = c - np.where(x < 0.08, x - 6.25 * x * x, 0.04)
    peak = c.max(-1, keepdims=True)
    d = 1.0 - start
    new_peak = 1.0 - d * d / (peak + d - start)
    comp = c * (new_peak / np.maximum(peak, 1e-30))
    g = 1.0 - 1.0 / (desat * (peak - new_peak) + 1.0)
    comp = comp + (new_peak - comp) * g
    return _srgb(np.where(peak < start, c, comp))


OPERATORS = {"filmic": _filmic, "uncharted": _uncharted, "clip": lambda c: _srgb(np.maximum(c, 0.0)), "aces": _aces, "agx": _agx, "khronos_pbr": _khronos}


def _reference(img, method, exposure=1.0, brightness=1.0, contrast=1.0, saturation=1.0, vignette=0.0):
    H, W, _ = img.shape
    c = OPERATORS[method](img[..., :3].astype(np.float64) * exposure)
    c = np.clip(0.5 + (c - 0.5) * contrast, 0.0, 1.0) ** (1.0 / brightness)
    luma = (c * np.array([0.299, 0.587, 0.114])).sum(-1, keepdims=True)
    c = luma + (c - luma) * saturation
    u = ((np.arange(W) + 0.5) / W - 0.5) * 2.0
    v = ((np.arange(H) + 0.5) / H - 0.5) * 2.0
    c = c * (1.0 - (u[None, :] ** 2 + v[:, None] ** 2) * vignette)[..., None]
    out = np.empty((H, W, 4), np.float64)
    out[..., :3] = c
    out[..., 3] = img[..., 3]
    return np.clip(out, 0.0, 1.0) * 255.0


def _tracer_with_image(assets, img):
    """A PathTracer whose accumulator holds `img` (mi_pt_write_accum)."""
    H, W, _ = img.shape
    scene = ptmod.Scene(os.path.join(assets, "Box.glb"))
    t = ptmod.PathTracer(scene)
    t.resize(W, H)
    t.write_accum(img)
    return t, None


@pytest.mark.parametrize("method", capi.TONEMAP_METHODS)
def test_operators_match_published_forms(built, assets, method):
    rng = np.random.default_rng(7)
    H, W = 96, 160
    img = np.empty((H, W, 4), np.float32)
    img[..., :3] = np.exp2(rng.uniform(-14.0, 5.0, (H, W, 3))).astype(np.float32)  # 19 stops, every channel on its own
    img[0, :16, :3] = 0.0  # black, and a few exact greys / saturated primaries
    img[1, :16, :3] = np.linspace(0.0, 4.0, 16, dtype=np.float32)[:, None]
    img[2, :3, :3] = np.eye(3, dtype=np.float32) * 3.0
    img[..., 3] = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    t, keep = _tracer_with_image(assets, img)
    for kw in (dict(), dict(exposure=2.5, brightness=1.3, contrast=0.8, saturation=1.4, vignette=0.35)):
        got = t.tonemap(method=method, **kw).astype(np.float64)
        want = _reference(img, method, **kw)
        diff = np.abs(got - np.floor(want + 0.5))
        # float32 vs float64 may land on the other side of a rounding boundary: allow one code, and only near a boundary
        assert diff.max() <= 1.0, (method, kw, diff.max())
        near = np.abs((want % 1.0) - 0.5) < 2e-2
        assert (diff[~near] == 0).all(), (method, kw, int((diff[~near] != 0).sum()))
        assert (diff != 0).mean() < 5e-3
    t.close()
    del keep


def test_inactive_passes_through_and_bad_arguments(built, assets):
    rng = np.random.default_rng(3)
    img = rng.uniform(-0.2, 1.4, (32, 48, 4)).astype(np.float32)
    t, keep = _tracer_with_image(assets, img)
    got = t.tonemap(isActive=0)
    assert (got == np.floor(np.clip(img.astype(np.float64), 0, 1) * 255.0 + 0.5)).all()
    with pytest.raises(ptmod.MiError):
        t.tonemap(method=9)
    with pytest.raises(ptmod.MiError):
        t.tonemap(brightness=0.0)
    with pytest.raises(ptmod.MiError):
        t.tonemap(source=1)  # no denoise result yet
    t.close()
    del keep


def test_auto_exposure_meters_the_geometric_mean(built, assets):
    """autoExposure (the reference's default, src/resources.hpp:212): exposure scaled by key 0.18 / geometric-mean luminance, metered
    through a 256-bin log2 histogram over [evMin, evMax]; a uniformly brighter image therefore tonemaps to the same picture, and the
    exposure eases towards its target with 1 - exp(-dt * speed)."""
    rng = np.random.default_rng(11)
    H, W = 64, 64
    base = np.exp2(rng.uniform(-6.0, 2.0, (H, W, 1))).astype(np.float32) * np.ones((1, 1, 3), np.float32)
    img = np.concatenate([base, np.ones((H, W, 1), np.float32)], -1)
    tm = capi.MiTonemapperData()
    capi.pt_lib().mi_pt_default_tonemapper(tm, 1)
    assert (tm.method, tm.isActive, tm.exposure, tm.brightness, tm.contrast, tm.saturation, tm.vignette, tm.autoExposure) == (0, 1, 1.0, 1.0, 1.0, 1.0, 0.0, 1)
    t, keep = _tracer_with_image(assets, img)
    a = t.tonemap(tm, dt_seconds=-1.0).astype(np.int32)
    # the metered exposure: bins are (evMax - evMin) / 256 = 1/8 stop wide
    lum = (img[..., :3].astype(np.float64) * np.array([0.2126, 0.7152, 0.0722])).sum(-1)
    expo = 0.18 / np.exp2(np.log2(lum).mean())
    want = _reference(img, "filmic", exposure=expo)
    assert np.abs(a - np.floor(want + 0.5))[..., :3].max() <= 6  # histogram quantisation: a 1/16-stop error at most
    t.close()
    del keep
    t2, keep2 = _tracer_with_image(assets, img * np.array([8.0, 8.0, 8.0, 1.0], np.float32))
    b = t2.tonemap(tm, dt_seconds=-1.0).astype(np.int32)
    assert np.abs(a - b).max() <= 1  # 3 stops brighter = exactly 24 bins up: the same picture
    # easing: one step of dt = ln 2 / speed moves the exposure half way to the new target
    t2.write_accum(img * np.array([2.0, 2.0, 2.0, 1.0], np.float32))
    c = t2.tonemap(tm, dt_seconds=float(np.log(2.0)) / tm.autoExposureSpeed).astype(np.int32)
    want_c = _reference(img * 2.0, "filmic", exposure=(expo / 8.0 + (expo / 2.0 - expo / 8.0) * 0.5))
    assert np.abs(c - np.floor(want_c + 0.5))[..., :3].max() <= 6
    t2.close()
    del keep2


# ---- ragged pixel counts, tail blocks, and auto exposure against the kernel's own definition ---------------------------------------------------
# Every linear-index launch above has W * H a multiple of 256; the tests below run k_tonemap with a partial last block (1, 255 and 259 pixels),
# k_lum_histogram round its grid-stride loop twice, and compare the metered exposure with a restatement of the 256-bin histogram the kernel
# builds -- to one 8-bit code, where the continuous geometric mean above needs six.
def _assert_picture(got, want, label, skip=None):
    """The assertions of test_operators_match_published_forms; `skip` (H, W) leaves pixels out."""
    diff = np.abs(got.astype(np.float64) - np.floor(want + 0.5))
    near = np.abs((want % 1.0) - 0.5) < 2e-2
    if skip is not None:
        diff, near = diff[~skip], near[~skip]
    print(f"TONEMAP_ROW | {label} | max {diff.max():.0f} code | {int((diff != 0).sum())} of {diff.size} values differ |")
    assert diff.max() <= 1.0, (label, diff.max())
    assert (diff[~near] == 0).all(), (label, int((diff[~near] != 0).sum()))
    assert (diff != 0).mean() < 5e-3, label


def _float32_stays_inside_the_share(want, label):
    """CPU side: float32 evaluation of these operators ends within 1e-3 code of the float64 value (relative error of a few 1e-6 on a value of at
    most 255), so only values that close to a rounding boundary can come out a code apart: their share must stay under the 5e-3 allowed."""
    risky = np.abs((want % 1.0) - 0.5) < 1e-3
    assert risky.mean() < 5e-3, (label, risky.mean())


RAGGED = ((1, 1), (255, 1), (7, 37))  # (W, H): 1, 255 and 259 = 256 + 3 pixels


@pytest.mark.parametrize("size", RAGGED, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("method", capi.TONEMAP_METHODS)
def test_operators_at_ragged_pixel_counts(built, assets, method, size):
    W, H = size
    rng = np.random.default_rng(1000 + 37 * W + H)
    img = np.empty((H, W, 4), np.float32)
    img[..., :3] = np.exp2(rng.uniform(-14.0, 5.0, (H, W, 3))).astype(np.float32)
    if W * H > 16:
        flat = img.reshape(-1, 4)
        flat[-1, :3] = 0.0  # the very last pixel of the tail block, black; exact greys just before it
        flat[-9:-1, :3] = np.linspace(0.0, 4.0, 8, dtype=np.float32)[:, None]
    img[..., 3] = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    t, keep = _tracer_with_image(assets, img)
    try:
        for kw in (dict(), dict(exposure=2.5, brightness=1.3, contrast=0.8, saturation=1.4, vignette=0.35)):
            want = _reference(img, method, **kw)
            _float32_stays_inside_the_share(want, (method, size))
            _assert_picture(t.tonemap(method=method, **kw), want, (method, size, kw))
    finally:
        t.close()
    del keep


def test_tail_block_of_the_passthrough_and_of_the_denoised_source(built, assets):
    """7 x 37 = 259 pixels: isActive = 0, and source = 1 after an a-trous run on a written image (the internal guide images are zero-filled, so the
    run is the colour term alone over one all-background image)."""
    from denoise_ref import atrous_iteration
    rng = np.random.default_rng(21)
    W, H = 7, 37
    img = rng.uniform(-0.2, 1.4, (H, W, 4)).astype(np.float32)
    t, keep = _tracer_with_image(assets, img)
    try:
        got = t.tonemap(isActive=0)
        assert (got == np.floor(np.clip(img.astype(np.float64), 0, 1) * 255.0 + 0.5)).all()
        albedo, normal = t.read_guides()
        assert not albedo.any() and not normal.any()
        den = t.denoise(iterations=1, sigma_color=1.0, sigma_normal=0.0, sigma_albedo=1e18)
        want_den, bound = atrous_iteration(img, albedo, normal, 1, 1.0, 0.0, 1e18, bound=True)
        assert (np.abs(den[..., :3] - want_den[..., :3]) <= bound).all() and np.array_equal(den[..., 3], img[..., 3])
        want = _reference(den, "clip")  # (of the device's own float32 result: this half is about the tonemapper reading the other buffer)
        _float32_stays_inside_the_share(want, "source=1")
        _assert_picture(t.tonemap(source=1, method="clip"), want, "source=1")
        _assert_picture(t.tonemap(source=0, method="clip"), _reference(img, "clip"), "source=0")
    finally:
        t.close()
    del keep


def _bin_centre(b, ev_min=-24.0, ev_max=8.0):
    """grey level whose log2 luminance sits in the middle of histogram bin b (fractional b allowed: below 0 or above 255 is outside the range)"""
    return np.exp2(ev_min + (np.asarray(b, np.float64) + 0.5) / 256.0 * (ev_max - ev_min))


def _grey(lum, alpha=1.0):
    lum = np.asarray(lum, np.float64)
    return np.concatenate([np.repeat(lum[..., None], 3, -1), np.full(lum.shape + (1,), alpha)], -1).astype(np.float32)


def _metered_exposure(img, ev_min=-24.0, ev_max=8.0, centre=False):
    """k_lum_histogram + k_auto_exposure restated: float32 luminance and log2, bin = int(t * 256) clamped to [0, 255], bin 0 dropped (it collects
    everything below evMin), the central disc of radius 1/4 counted four times, exposure = 0.18 / 2^(sum(w ev) / sum(w)) in float64; 1 when nothing
    is metered.  Also asserts what makes the comparison sharp: every metered pixel at least a quarter bin from a bin edge and at least 1e-4 from
    the disc boundary in du^2 + dv^2."""
    H, W, _ = img.shape
    f = np.float32
    c = img[..., :3].astype(f)
    lum = f(0.2126) * c[..., 0] + f(0.7152) * c[..., 1] + f(0.0722) * c[..., 2]
    with np.errstate(invalid="ignore"):
        ok = lum > 0  # (false for NaN)
    t = (np.log2(lum[ok]) - f(ev_min)) / (f(ev_max) - f(ev_min))
    pos = t.astype(np.float64) * 256.0
    b = np.clip(np.trunc(t * f(256.0)), 0, 255).astype(np.int64)
    edge = np.clip(np.round(pos), 1, 255)  # (the edges that separate bins: 1 .. 255)
    assert (np.abs(pos - edge) >= 0.25).all(), "a pixel within a quarter bin of a bin edge"
    w = np.ones((H, W))
    if centre:
        y, x = np.mgrid[0:H, 0:W]
        du, dv = (x.astype(f) + f(0.5)) / f(W) - f(0.5), (y.astype(f) + f(0.5)) / f(H) - f(0.5)
        r2 = du * du + dv * dv
        assert (np.abs(r2.astype(np.float64) - 0.0625)[ok] >= 1e-4).all(), "a metered pixel on the disc boundary"
        w = np.where(r2 < f(0.0625), 4.0, 1.0)
    hist = np.bincount(b, weights=w[ok], minlength=256)
    hist[0] = 0.0
    ev = ev_min + (np.arange(256) + 0.5) / 256.0 * (ev_max - ev_min)
    return (0.18 / np.exp2((hist * ev).sum() / hist.sum()) if hist.sum() > 0 else 1.0), hist


def _auto_tm(**fields):
    tm = capi.MiTonemapperData()
    capi.pt_lib().mi_pt_default_tonemapper(tm, 1)
    tm.method = capi.TONEMAP_METHODS.index("clip")
    for k, v in fields.items():
        setattr(tm, k, v)
    return tm


def _assert_exposed(t, img, tm, exposure, label, dt=-1.0, skip=None, readable=50):
    """The exposure has no getter: it is read from the picture.  Under `clip`, over exposed values in [0.05, 1], one 8-bit code is under 2 % of
    exposure while one histogram bin is 9 %: the picture is held to one code, and must hold enough such pixels to tell."""
    exposed = img[..., 0].astype(np.float64) * exposure
    with np.errstate(invalid="ignore"):
        assert ((exposed >= 0.05) & (exposed <= 1.0)).sum() >= readable, label
    want = _reference(np.nan_to_num(img), "clip", exposure=exposure)
    _float32_stays_inside_the_share(want if skip is None else want[~skip], label)
    _assert_picture(t.tonemap(tm, dt_seconds=dt), want, label, skip)


def _planted_cases():
    """name -> (image, tonemapper fields, pixels left out of the picture comparison or None)"""
    rng = np.random.default_rng(31)
    W, H = 40, 24
    y, x = np.mgrid[0:H, 0:W]
    cases = {}
    # 1. plain: bins between -7 and +1 EV
    cases["plain"] = (_grey(_bin_centre(rng.integers(136, 200, (H, W)))), {}, None)
    # 2. centre metering: the disc of radius 1/4 (in du^2 + dv^2 < 1/16) counts four times
    r2 = ((x + 0.5) / W - 0.5) ** 2 + ((y + 0.5) / H - 0.5) ** 2
    disc = r2 < 0.0625
    dark, bright = rng.integers(144, 160, (H, W)), rng.integers(168, 184, (H, W))
    cases["centre-dark-disc"] = (_grey(_bin_centre(np.where(disc, dark, bright))), dict(enableCenterMetering=1), None)
    cases["centre-bright-disc"] = (_grey(_bin_centre(np.where(disc, bright, dark))), dict(enableCenterMetering=1), None)
    # 3. evMin / evMax = -8 / 4: pixels below the range (bin 0: dropped), inside it and above it (clamped into bin 255)
    kind = rng.choice(3, (H, W), p=[0.2, 0.7, 0.1])
    inside = rng.integers(64, 150, (H, W))  # -5 .. -1 EV at 12 / 256 EV a bin
    lum = _bin_centre(np.where(kind == 0, -40.0 - inside, np.where(kind == 1, inside, 300.0 + inside)), -8.0, 4.0)
    cases["ev-range"] = (_grey(lum), dict(evMinValue=-8.0, evMaxValue=4.0), None)
    # 4. zero, negative and NaN luminance: skipped by the meter; only those pixels are left out of the picture comparison
    img = _grey(_bin_centre(rng.integers(136, 200, (H, W))))
    bad = rng.choice(4, (H, W), p=[0.85, 0.05, 0.05, 0.05])
    img[bad == 1, :3] = 0.0
    img[bad == 2, :3] = np.float32([-0.5, -2.0, 0.25])  # (luminance -1.5)
    img[bad == 3, :3] = np.nan
    cases["unmeterable-pixels"] = (img, {}, bad != 0)
    # 5. nothing to meter: every pixel below evMin (bin 0) or black: factor 1
    img = _grey(_bin_centre(-8.0 - rng.integers(0, 24, (H, W)), -2.0, 8.0))  # 0.06 .. 0.23: readable at exposure 1
    img[::5, ::3, :3] = 0.0
    cases["nothing-metered"] = (img, dict(evMinValue=-2.0, evMaxValue=8.0), None)
    return cases


@pytest.mark.parametrize("name", ["plain", "centre-dark-disc", "centre-bright-disc", "ev-range", "unmeterable-pixels", "nothing-metered"])
def test_auto_exposure_equals_the_histogram_it_builds(built, assets, name):
    img, fields, skip = _planted_cases()[name]
    tm = _auto_tm(**fields)
    exposure, hist = _metered_exposure(img, tm.evMinValue, tm.evMaxValue, bool(tm.enableCenterMetering))
    if name == "nothing-metered":
        assert exposure == 1.0 and hist.sum() == 0
    elif name == "ev-range":
        assert hist[255] > 0 and hist[1:255].sum() > 0
    elif name.startswith("centre"):
        flat, _ = _metered_exposure(img, tm.evMinValue, tm.evMaxValue, False)
        assert abs(np.log2(flat / exposure)) > 0.25  # the disc's weight moves the exposure by more than a quarter stop: 12 % against 2 % a code
    t, keep = _tracer_with_image(assets, img)
    try:
        _assert_exposed(t, img, tm, exposure, name, skip=skip)
    finally:
        t.close()
    del keep


def test_auto_exposure_jumps_holds_and_eases(built, assets):
    """dt < 0 jumps to the target, dt = 0 keeps the previous exposure, one step of dt = ln 2 / speed then moves half way."""
    rng = np.random.default_rng(42)  # (a seed at which none of the 64 grey levels lands next to a rounding boundary at any of the three exposures)
    W, H = 40, 24
    img_a = _grey(_bin_centre(rng.integers(136, 200, (H, W))))
    img_b = _grey(_bin_centre(rng.integers(168, 200, (H, W))))  # two stops brighter on average
    tm = _auto_tm()
    e_a, _ = _metered_exposure(img_a)
    e_b, _ = _metered_exposure(img_b)
    assert abs(np.log2(e_a / e_b)) > 0.25
    t, keep = _tracer_with_image(assets, img_a)
    try:
        _assert_exposed(t, img_a, tm, e_a, "jump")
        t.write_accum(img_b)
        _assert_exposed(t, img_b, tm, e_a, "hold", dt=0.0)
        _assert_exposed(t, img_b, tm, e_a + (e_b - e_a) * 0.5, "half-life", dt=float(np.log(2.0)) / tm.autoExposureSpeed)
    finally:
        t.close()
    del keep


def test_histogram_stride_loop_goes_round_twice(built, assets):
    """1024 x 513 = 525 312 pixels, more than the 2048 x 256 the capped grid covers in one pass: every pixel is below evMin (bin 0) except the last
    row, so a loop that stops after one pass meters nothing and returns factor 1."""
    rng = np.random.default_rng(51)
    W, H = 1024, 513
    assert W * H > 2048 * 256 and W * (H - 1) == 2048 * 256
    lum = np.full((H, W), 2.0 ** -30)
    lum[-1] = _bin_centre(rng.integers(184, 200, W))  # -1 .. +1 EV: exposure 0.18 or so, far from 1
    img = _grey(lum)
    tm = _auto_tm()
    exposure, hist = _metered_exposure(img)
    assert hist.sum() == W and abs(np.log2(exposure)) > 0.25
    t, keep = _tracer_with_image(assets, img)
    try:
        _assert_exposed(t, img, tm, exposure, "stride", readable=W // 2)
    finally:
        t.close()
    del keep
