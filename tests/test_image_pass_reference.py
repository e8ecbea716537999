"""CPU tier of the image-pass tests: proves the references (tests/denoise_ref.py) and the cases (tests/image_pass_cases.py) before the device sees
them (tests/test_gpu_image_passes.py), and prints the tolerance each device comparison will use."""
import numpy as np
import pytest

import denoise_ref as ref
import image_pass_cases as ipc

STRUCTURAL = [c for c in ipc.all_cases() if c.tier == "structural"]


def _exact(case):
    """The structural case through the rational filter: weights are 1 or 0 by the hit-fraction kind and, with axis normals, the sign of the dot."""
    H, W = case.H, case.W
    solid = (case.albedo[..., 3] > np.float32(0.5)).tolist()
    values = [[[int(v) for v in case.color[y, x, :3]] for x in range(W)] for y in range(H)]
    passes = None
    if case.axis_normals:
        n = case.normal[..., :3].astype(int).tolist()

        def passes(y, x, qy, qx):
            return (not solid[y][x]) or sum(p * q for p, q in zip(n[y][x], n[qy][qx])) > 0
    img = ref.exact_filter(values, solid, case.iterations, passes, centre_always=case.kind != "atrous")
    return img


@pytest.mark.parametrize("case", STRUCTURAL, ids=lambda c: c.name)
def test_float64_restatement_equals_the_exact_rational_filter(case):
    """Exact where sums and quotients are representable, within 2 ulp of float64 elsewhere."""
    assert (case.color[..., :3] == np.round(case.color[..., :3])).all() and (case.albedo[..., :3] == 1).all()
    want = ipc.restate(case)
    exact = _exact(case)
    fl = np.array([[[float(v) for v in px] for px in row] for row in exact])
    representable = np.array([[[float(v) == v for v in px] for px in row] for row in exact])
    ulps = np.abs(want[..., :3] - fl) / np.spacing(np.maximum(np.abs(fl), 1e-300))
    print(f"{case.name}: max {ulps.max():.2f} ulp, {int(representable.sum())} of {representable.size} exact values representable, "
          f"{int((ulps[representable] == 0).sum())} of them met exactly")
    assert ulps.max() <= 2.0, ulps.max()
    assert np.array_equal(want[..., 3], case.color[..., 3].astype(np.float64))  # alpha untouched


def _random_guides(rng, W, H):
    a = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)
    a[..., 3] = ipc.hit_fraction("blocks", W, H, rng)[0]
    n = ipc._unit_normals(rng, W, H, 0.3)
    n[..., 3] = rng.uniform(0.0, 9.0, (H, W))
    d = (0.9 + 0.002 * np.mgrid[0:H, 0:W][1] + 0.001 * rng.uniform(0, 1, (H, W))).astype(np.float32)
    return a, n, d


@pytest.mark.parametrize("sigmas", [(0.6, 64.0, 0.2), (0.0, 1.0, 0.0), (ipc.OFF, 0.0, ipc.OFF)])
def test_partition_of_unity(sigmas):
    """A constant image comes back unchanged for any sigmas (normalised weights); SVGF demodulates and re-modulates, so to a few float64 ulp."""
    rng = np.random.default_rng(5)
    W, H = 17, 33
    a, n, d = _random_guides(rng, W, H)
    img = np.full((H, W, 4), 2.5, np.float32) * np.float32([1.0, 0.5, 0.25, 0.3])
    got = ref._atrous_numpy(img, a, n, 3, *sigmas)
    assert np.abs(got - img).max() <= 4 * np.spacing(2.5)
    a[..., :3] = 0.5  # a constant demodulated image needs a constant albedo
    for frames in (1, 8):
        got = ref._svgf_numpy(img, a, n, d, frames, 3, max(sigmas[0], 0.5), sigmas[1], max(sigmas[2], 0.5))
        assert np.abs(got - img).max() <= 8 * np.spacing(2.5)


def _flip(arrs, op):
    return [np.ascontiguousarray(op(x)) for x in arrs]


def test_flips_and_transposition_commute_with_the_filters():
    """Flipping or transposing all inputs flips or transposes the output.  SVGF's depth gradient is a FORWARD difference, which a flip turns into
    a backward one: SVGF is flipped with a constant depth and transposed with a varying one."""
    rng = np.random.default_rng(6)
    W, H = 17, 33
    a, n, d = _random_guides(rng, W, H)
    img = rng.uniform(0.0, 3.0, (H, W, 4)).astype(np.float32)
    flat = np.full_like(d, 0.75)
    ops = {"flip-x": lambda x: x[:, ::-1], "flip-y": lambda x: x[::-1], "transpose": lambda x: np.swapaxes(x, 0, 1)}
    base_a = ref._atrous_numpy(img, a, n, 3, 0.6, 64.0, 0.2)
    for name, op in ops.items():
        fi, fa, fn = _flip((img, a, n), op)
        assert np.abs(ref._atrous_numpy(fi, fa, fn, 3, 0.6, 64.0, 0.2) - op(base_a)).max() <= 1e-12, name
        for frames in (1, 8):
            dep = d if name == "transpose" else flat
            base_s = ref._svgf_numpy(img, a, n, dep, frames, 3, 4.0, 128.0, 1.0)
            fd, = _flip((dep,), op)
            assert np.abs(ref._svgf_numpy(fi, fa, fn, fd, frames, 3, 4.0, 128.0, 1.0) - op(base_s)).max() <= 1e-12, (name, frames)


def test_single_iteration_entry_point_returns_the_intermediate():
    c = next(c for c in ipc.all_cases() if c.name == "svgf-lum-variance-17x33")
    out, bound, inter = ref.svgf_single(c.color, c.albedo, c.normal, c.depth, c.ref_frames, *c.sigmas)
    assert np.array_equal(out, ipc.restate(c)) and inter.shape == (c.H, c.W, 4) and (bound > 0).all()
    cur, dem = ref.svgf_prepare(c.color, c.albedo, c.normal, c.ref_frames)
    # the variance channel is sum(h^2 var) / sum(h)^2 with sum(h^2) <= sum(h)^2: never above the largest input variance, never negative
    assert (inter[..., 3] <= cur[..., 3].max() + 1e-12).all() and (inter[..., 3] >= 0).all()
    assert np.abs(inter[..., :3] * dem - out[..., :3]).max() <= 1e-12


def test_two_iteration_case_sees_the_variance_channel():
    """The variance filtered with h^2 and divided by sw^2 does not show in the output of one iteration; the two-iteration case must move by far
    more than its bound when the first iteration's variance comes out wrong by the factor a forgotten square gives."""
    c = next(c for c in ipc.all_cases() if c.name == "svgf-lum-two-iterations-17x33")
    want, bound, _ = ipc.expected(c)
    cur, dem = ref.svgf_prepare(c.color, c.albedo, c.normal, c.ref_frames)
    first = ref.svgf_iteration(cur, c.albedo, c.normal, c.depth, 1, *c.sigmas)
    wrong = first.copy()
    wrong[..., 3] *= 2.0  # (sum(h) is between 9/64 and 1: dividing by sw instead of sw^2 is off by 1 to 7)
    moved = ref.svgf_finish(ref.svgf_iteration(wrong, c.albedo, c.normal, c.depth, 2, *c.sigmas), dem, c.color.astype(np.float64)).astype(np.float64)
    assert ipc.worst(moved, want, bound)[0] > 10.0


def test_case_conditions_hold_with_no_ambiguous_pixel():
    for c in ipc.all_cases():
        assert (c.W, c.H) in ipc.SIZES and (c.W != c.H or c.W == 1), c.name
        for op in (lambda x: x[:, ::-1], lambda x: x[::-1]):  # never mirror-symmetric (one-pixel-wide axes have no mirror image to differ from)
            if c.color[..., :3].size > 3 and not (c.W == 1 and c.H == 1):
                assert not np.array_equal(op(c.color), c.color) or min(c.W, c.H) == 1, c.name
        hf = c.albedo[..., 3]
        near = np.abs(hf.astype(np.float64) - 0.5) < 1e-6
        assert np.array_equal(near, c.planted_half), c.name  # no hit fraction next to 0.5 other than the planted values
        assert set(np.unique(hf[near]).tolist()) <= {0.5, float(ipc.HALF_UP)}, c.name
        if c.kind == "atrous":
            continue
        solid = hf > np.float32(0.5)
        lum_on = c.sigmas[0] != ipc.OFF
        if c.spatial and lum_on:  # the > 0.9 test of the 7x7 estimate: no dot product of two geometry pixels 3 apart or less within 1e-3 of 0.9
            n = c.normal[..., :3].astype(np.float64)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    qy, qx, valid = ref._gather(c.H, c.W, dy, dx)
                    dot = (n[qy][:, qx] * n).sum(-1)
                    both = valid & solid & solid[qy][:, qx]
                    assert not (both & (np.abs(dot - 0.9) < 1e-3)).any(), (c.name, dy, dx)
        if not lum_on and c.W * c.H > 1:  # the luminance term is off only where the prefiltered variance is positive
            cur, _ = ref.svgf_prepare(c.color, c.albedo, c.normal, c.ref_frames)
            nxt = ref.svgf_iteration(cur, c.albedo, c.normal, c.depth, 1, *c.sigmas)
            assert np.isfinite(nxt).all(), c.name
            gv = np.zeros((c.H, c.W))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qy, qx, valid = ref._gather(c.H, c.W, dy, dx)
                    gv += valid * cur[qy][:, qx][..., 3]
            assert (gv > 1e-6).all(), c.name
        if c.name.startswith("svgf-lum-variance") or (c.name.startswith("svgf-prepare-frames") and not c.spatial):
            cur, _ = ref.svgf_prepare(c.color, c.albedo, c.normal, c.ref_frames)
            assert (cur[..., 3] > 0).all(), c.name
    d = ipc.PREPARE_DIRECTIONS
    dots = (d[:, None, :] * d[None, :, :]).sum(-1)
    assert (np.abs(dots - 0.9) >= 1e-3).all() and np.allclose(np.diag(dots), 1.0)


def test_print_the_tolerances_and_hold_the_float32_restatement_to_them():
    """The tolerance each device comparison will use, and the same comparison made on the CPU: the float32 restatement, in the kernel's operation
    order, must sit inside the bound derived for float32 arithmetic (structural and numerical tiers; the joint bound is defined from it)."""
    print(f"{'case':52s} {'cpu discrepancy':>16s} {'bound (max)':>12s} {'worst ratio':>12s}")
    for c in ipc.all_cases():
        want, bound, disc = ipc.expected(c)
        f32 = ipc.restate(c, np.float32)
        ratio, err, b, where, border = ipc.worst(f32, want, bound)
        print(f"{c.name:52s} {disc:16.3e} {bound.max():12.3e} {ratio:12.3f}")
        assert np.array_equal(f32[..., 3], c.color[..., 3])
        assert ratio <= 1.0, (c.name, ratio, err, b, where, border)
