"""Synthetic inputs for the denoise kernels (csrc/device/denoise.hip): small, seeded, never square and never mirror-symmetric, built so that
the expected result is known almost exactly.  Shared by tests/test_image_pass_reference.py (CPU: proves the cases and the references),
tests/image_pass_device_child.py (runs them on the device) and tests/test_gpu_image_passes.py (compares).

A case is a `Case`: the four images, the entry point (`atrous` = mi_pt_denoise, `svgf` = mi_pt_denoise_svgf, `temporal` = mi_pt_denoise_temporal
with an empty history), its arguments and how the accumulator gets its frames:
    frames == 1                the accumulator is written through mi_pt_write_accum: SVGF estimates the variance spatially
    frames  > 1                `frames` frames of Box.glb are rendered with the guides on, then the bound tensors are overwritten: the moment
                               covers the frames, so from 4 on the variance comes from the second moment in normal.w
    rewrite                    as frames > 1, but the accumulator is then written through mi_pt_write_accum: spatial again
tier: `structural` (every weight exactly 0 or 1), `numerical` (one edge-stopping term, one iteration), `joint` (everything on)."""
import numpy as np

OFF = 1e18  # a sigma that switches its term off: the argument of the exp underflows to 0
SIZES = ((1, 1), (1, 37), (37, 1), (17, 33), (48, 35))  # (W, H): the kernels tile 16 x 16
HALF_UP = np.nextafter(np.float32(0.5), np.float32(1.0))
PATTERNS = ("all_geometry", "all_background", "checker", "single_geometry", "single_background", "diagonal", "exact_half", "blocks")


class Case:
    def __init__(self, name, tier, kind, color, albedo, normal, depth, iterations, sigmas, frames=1, rewrite=False, planted_half=None, axis_normals=False):
        self.name, self.tier, self.kind = name, tier, kind
        self.color, self.albedo, self.normal, self.depth = (np.array(x, np.float32, order="C") for x in (color, albedo, normal, depth))  # (copies)
        self.iterations, self.sigmas, self.frames, self.rewrite = iterations, tuple(float(s) for s in sigmas), frames, rewrite
        self.planted_half = planted_half if planted_half is not None else np.zeros(self.depth.shape, bool)
        self.axis_normals = axis_normals
        self.H, self.W = self.depth.shape

    @property
    def spatial(self):
        return self.frames < 4 or self.rewrite

    @property
    def ref_frames(self):
        """what k_svgf_prepare is given: the frame count when the moment covers the frames, 1 otherwise"""
        return 1 if (self.rewrite or self.frames == 1) else self.frames


def hit_fraction(pattern, W, H, rng):
    """(hit fraction image, mask of the planted exact values 0.5 and nextafter(0.5, 1))"""
    y, x = np.mgrid[0:H, 0:W]
    planted = np.zeros((H, W), bool)
    if pattern == "all_geometry":
        solid = np.ones((H, W), bool)
    elif pattern == "all_background":
        solid = np.zeros((H, W), bool)
    elif pattern == "checker":
        solid = ((x + y) & 1) == 0
    elif pattern in ("single_geometry", "single_background"):
        solid = np.zeros((H, W), bool)
        solid[H // 3, W // 4] = True
        if pattern == "single_background":
            solid = ~solid
    elif pattern == "diagonal":
        solid = 5 * x * max(H, 2) > 4 * y * max(W, 2) + 3
    elif pattern == "blocks":
        solid = ((x // 3 + 2 * (y // 5)) % 3) != 0
    else:  # exact_half
        solid = rng.random((H, W)) < 0.5
    hf = np.where(solid, rng.choice(np.float32([1.0, 0.75, 0.625]), (H, W)), rng.choice(np.float32([0.0, 0.25, 0.375]), (H, W))).astype(np.float32)
    if pattern == "exact_half":
        planted = rng.random((H, W)) < 0.3
        hf = np.where(planted, np.where(solid, HALF_UP, np.float32(0.5)), hf).astype(np.float32)  # 0.5 itself is background: the test is > 0.5
    return hf, planted


def _rgba(rgb, rng):
    H, W, _ = rgb.shape
    return np.concatenate([rgb, rng.uniform(0.0, 1.0, (H, W, 1))], -1).astype(np.float32)  # alpha: anything, it must come back bit for bit


AXES = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0]])


def _structural(kind, W, H, pattern, iterations, seed, axis=False):
    rng = np.random.default_rng(seed)
    hf, planted = hit_fraction(pattern, W, H, rng)
    color = _rgba(rng.integers(0, 10, (H, W, 3)).astype(np.float32), rng)
    albedo = np.concatenate([np.ones((H, W, 3), np.float32), hf[..., None]], -1)
    normal = np.zeros((H, W, 4), np.float32)
    if axis:  # the six axis directions and, on an eighth of the pixels, the zero vector: every dot product is -1, 0 or 1
        normal[..., :3] = AXES[rng.choice(7, (H, W), p=[0.1, 0.1, 0.1, 0.1, 0.375, 0.1, 0.125])]
    else:
        normal[..., 2] = 1.0
    normal[..., 3] = rng.uniform(0.0, 100.0, (H, W))  # (the second moment: not read on the spatial route)
    depth = np.full((H, W), 0.75, np.float32)  # depthKey = 4 exactly, gradient 0
    sig_n = 0.0 if not axis else (64.0 if kind == "atrous" else 128.0)
    sigmas = (OFF, sig_n, OFF)  # atrous: colour, normal, albedo; svgf: luminance, normal, depth
    name = f"{kind}-{'axis' if axis else 'mask'}-{pattern}-{W}x{H}-it{iterations}"
    return Case(name, "structural", kind, color, albedo, normal, depth, iterations, sigmas, planted_half=planted, axis_normals=axis)


def structural_cases():
    out = []
    for kind in ("atrous", "svgf"):
        seed = 100 if kind == "atrous" else 200
        for it in range(1, 9):  # iterations 1..8 on 17 x 33: both ping-pong parities, steps up to 128 where most taps fall outside
            out.append(_structural(kind, 17, 33, PATTERNS[it - 1], it, seed + it))
        out.append(_structural(kind, 48, 35, "checker", 3, seed + 11))
        out.append(_structural(kind, 48, 35, "exact_half", 4, seed + 12))
        out.append(_structural(kind, 48, 35, "single_geometry", 5, seed + 13))
        out.append(_structural(kind, 1, 1, "all_geometry", 2, seed + 14))
        out.append(_structural(kind, 1, 37, "checker", 3, seed + 15))
        out.append(_structural(kind, 37, 1, "diagonal", 4, seed + 16))
        out.append(_structural(kind, 17, 33, "blocks", 3, seed + 17, axis=True))
        out.append(_structural(kind, 48, 35, "diagonal", 2, seed + 18, axis=True))
    for W, H, pattern, seed in ((17, 33, "blocks", 301), (48, 35, "exact_half", 302)):
        c = _structural("svgf", W, H, pattern, 3, seed)
        out.append(Case(c.name.replace("svgf-", "temporal-"), "structural", "temporal", c.color, c.albedo, c.normal, c.depth, 3, c.sigmas, frames=2,
                        planted_half=c.planted_half))
    return out


def _unit_normals(rng, W, H, spread):
    n = np.zeros((H, W, 4))
    v = rng.normal(0.0, spread, (H, W, 3)) + np.array([0.2, -0.1, 1.0])
    n[..., :3] = v / np.linalg.norm(v, axis=-1, keepdims=True)
    return n.astype(np.float32)


def _smooth(rng, W, H, ch, lo, hi):
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([np.sin(0.31 * x + 0.17 * y + k) * np.cos(0.11 * x - 0.23 * y + 2 * k) for k in range(ch)], -1)
    return (lo + (hi - lo) * (0.5 + 0.35 * base + 0.15 * rng.uniform(-1.0, 1.0, (H, W, ch)))).astype(np.float32)


def _guides(rng, W, H, pattern="blocks", albedo=None, normal=None, depth=None):
    hf, planted = hit_fraction(pattern, W, H, rng)
    a = np.ones((H, W, 4), np.float32) if albedo is None else np.concatenate([albedo, np.ones((H, W, 1), np.float32)], -1)
    a[..., 3] = hf
    if normal is None:
        normal = np.zeros((H, W, 4), np.float32)
        normal[..., 2] = 1.0
    if depth is None:
        depth = np.full((H, W), 0.75, np.float32)
    return a, normal.copy(), depth, planted


def _with_moment(color, albedo, normal, ratio):
    """normal.w = E[l^2] = l^2 (1 + ratio): ratio < 0 is the clamped negative variance"""
    l = (color[..., :3].astype(np.float64) * np.array([0.2126, 0.7152, 0.0722])).sum(-1)
    normal[..., 3] = (l * l * (1.0 + ratio)).astype(np.float32)
    return normal


def numerical_cases():
    out = []
    # ---- a-trous: one term each ------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(401)
    W, H = 17, 33
    a, n, d, _ = _guides(rng, W, H)
    # colour differences from 1e-3 to 12: weights from 1 - 1e-6 down to exp(-400) = 0
    col = 1.0 + rng.choice([0.0, 1e-3, 0.03, 0.3, 1.0, 3.0, 6.0, 12.0], (H, W, 1)) * rng.uniform(0.5, 1.0, (H, W, 3))
    out.append(Case("atrous-colour-17x33", "numerical", "atrous", _rgba(col, rng), a, n, d, 1, (1.0, 0.0, OFF)))
    W, H = 48, 35
    a, n, d, _ = _guides(rng, W, H, "diagonal")
    col = 1.0 + 1e-4 * rng.integers(0, 12, (H, W, 3))  # sigma_color = 0 is clamped to 1e-8: differences of 1e-4 are one unit of the argument
    out.append(Case("atrous-colour-sigma0-48x35", "numerical", "atrous", _rgba(col, rng), a, n, d, 1, (0.0, 0.0, OFF)))
    a, n, d, _ = _guides(rng, W, H, "blocks", albedo=rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32))
    out.append(Case("atrous-albedo-48x35", "numerical", "atrous", _rgba(rng.uniform(0.0, 4.0, (H, W, 3)), rng), a, n, d, 1, (OFF, 0.0, 0.2)))
    for s, spread in ((1.0, 1.0), (64.0, 0.15), (128.0, 0.1)):
        W, H = (17, 33) if s != 64.0 else (48, 35)
        a, n, d, _ = _guides(rng, W, H, "blocks", normal=_unit_normals(rng, W, H, spread))
        out.append(Case(f"atrous-normal{int(s)}-{W}x{H}", "numerical", "atrous", _rgba(rng.uniform(0.0, 4.0, (H, W, 3)), rng), a, n, d, 1, (OFF, s, OFF)))
    # ---- SVGF: one term each (spatial variance through mi_pt_write_accum unless the term needs the second moment) -------------------------
    rng = np.random.default_rng(402)
    W, H = 17, 33
    a, n, d, _ = _guides(rng, W, H, "blocks", normal=_unit_normals(rng, W, H, 0.1))
    out.append(Case("svgf-normal128-17x33", "numerical", "svgf", _rgba(rng.uniform(0.5, 4.0, (H, W, 3)), rng), a, n, d, 1, (OFF, 128.0, OFF)))
    y, x = np.mgrid[0:37, 0:48]
    depth_cases = {
        "ramp-x-48x35": (0.9 + 0.002 * x)[:35] + 0.0003 * rng.uniform(0, 1, (35, 48)),  # backward difference in the last column
        "ramp-y-17x33": (0.6 + 0.011 * y + 0.0002 * x)[:33, :17] + 0.0005 * rng.uniform(0, 1, (33, 17)),  # and in the last row
        "step-17x33": np.where(3 * x > 2 * y + 5, 0.95, 0.8)[:33, :17] + 0.001 * rng.uniform(0, 1, (33, 17)),
        "clamp-17x33": np.where(x + y < 12, 1.0, np.where(x > 11, 1.0 + 0.01 * y, 0.99 + 0.0002 * y))[:33, :17],  # 1.0 and > 1: depthKey = 1e7
        "column-1x37": (0.7 + 0.006 * y)[:37, :1] + 0.001 * rng.uniform(0, 1, (37, 1)),  # W = 1: the x difference is 0
        "row-37x1": (0.7 + 0.006 * x)[:1, :37] + 0.001 * rng.uniform(0, 1, (1, 37)),  # H = 1
    }
    for name, dep in depth_cases.items():
        H, W = dep.shape
        a, n, _, _ = _guides(rng, W, H, "single_background")
        out.append(Case(f"svgf-depth-{name}", "numerical", "svgf", _rgba(rng.uniform(0.5, 4.0, (H, W, 3)), rng), a, n, dep, 1, (OFF, 0.0, 1.0)))
    # luminance term: the variance through the second moment, so 4 rendered frames first
    W, H = 17, 33
    a, n, d, _ = _guides(rng, W, H, "blocks")
    col = _rgba(_smooth(rng, W, H, 3, 0.5, 3.0), rng)
    out.append(Case("svgf-lum-variance-17x33", "numerical", "svgf", col, a, _with_moment(col, a, n, rng.uniform(0.05, 3.0, (H, W))), d, 1, (4.0, 0.0, OFF), frames=4))
    # zero variance (m2 - l^2 negative everywhere: clamped): the weight is exp(-|dl| / 1e-6), luminances a few 1e-6 apart
    small = _rgba(1e-5 + 1e-6 * rng.integers(0, 6, (H, W, 1)) * np.ones((1, 1, 3)), rng)
    out.append(Case("svgf-lum-clamped-zero-17x33", "numerical", "svgf", small, a, _with_moment(small, a, n, np.full((H, W), -0.5)), d, 1, (4.0, 0.0, OFF), frames=4))
    # variance at border pixels only: the 3x3 prefilter renormalises there
    ratio = np.full((H, W), -0.5)
    ratio[0, 5], ratio[H - 1, W - 1], ratio[11, 0], ratio[20, W - 1] = 2.0, 1.0, 3.0, 0.5
    col = _rgba(1.0 + 0.02 * rng.integers(0, 8, (H, W, 1)) * np.ones((1, 1, 3)), rng)
    out.append(Case("svgf-lum-border-variance-17x33", "numerical", "svgf", col, a, _with_moment(col, a, n, ratio), d, 1, (4.0, 0.0, OFF), frames=4))
    # ---- the prepare step, seen through the luminance term ------------------------------------------------------------------------------------
    rng = np.random.default_rng(403)
    for frames in (3, 4, 16):
        alb = rng.uniform(0.1, 1.0, (H, W, 3)).astype(np.float32)
        alb[rng.random((H, W)) < 0.2] = np.float32([0.005, 0.019, 0.3])  # below the 0.02 floor
        a, n, d, _ = _guides(rng, W, H, "blocks", albedo=alb, normal=_prepare_normals(rng, W, H))
        col = _rgba(_smooth(rng, W, H, 3, 0.2, 2.0), rng)
        out.append(Case(f"svgf-prepare-frames{frames}-17x33", "numerical", "svgf", col, a, _with_moment(col, a, n, rng.uniform(0.1, 2.0, (H, W))), d, 1,
                        (4.0, 0.0, OFF), frames=frames))
    # the 7x7 estimate at image corners and with no neighbour of the same kind (single pixels of the other kind in the corners)
    W, H = 48, 35
    a, n, d, _ = _guides(rng, W, H, "all_geometry", normal=_prepare_normals(rng, W, H))
    for yy, xx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (17, 20)):
        a[yy, xx, 3] = 0.0
    out.append(Case("svgf-prepare-spatial-corners-48x35", "numerical", "svgf", _rgba(_smooth(rng, W, H, 3, 0.2, 2.0), rng), a, n, d, 1, (4.0, 0.0, OFF)))
    # the moment no longer covers the frames after mi_pt_write_accum: spatial although 16 frames were rendered
    W, H = 17, 33
    a, n, d, _ = _guides(rng, W, H, "diagonal", normal=_prepare_normals(rng, W, H))
    col = _rgba(_smooth(rng, W, H, 3, 0.2, 2.0), rng)
    out.append(Case("svgf-prepare-rewrite-17x33", "numerical", "svgf", col, a, _with_moment(col, a, n, rng.uniform(0.1, 2.0, (H, W))), d, 1, (4.0, 0.0, OFF),
                    frames=16, rewrite=True))
    return out


# unit directions whose pairwise dot products stay 1e-3 and more away from 0.9 (tests/test_image_pass_reference.py checks)
PREPARE_DIRECTIONS = np.float64([[0, 0, 1], [np.sin(0.3), 0, np.cos(0.3)], [0, np.sin(0.7), np.cos(0.7)], [-np.sin(0.55), 0, np.cos(0.55)]])


def _prepare_normals(rng, W, H):
    n = np.zeros((H, W, 4), np.float32)
    y, x = np.mgrid[0:H, 0:W]
    n[..., :3] = PREPARE_DIRECTIONS[(x // 4 + 3 * (y // 3) + rng.integers(0, 2, (H, W))) % 4]
    return n


def joint_cases():
    """All terms on, default sigmas; and the one two-iteration luminance case (the variance channel, filtered with h^2 and divided by sw^2, is
    invisible in the output of a single iteration)."""
    out = []
    rng = np.random.default_rng(501)
    for (W, H) in ((17, 33), (48, 35)):
        for it in (3, 5):
            alb = _smooth(rng, W, H, 3, 0.2, 0.9)
            y, x = np.mgrid[0:H, 0:W]
            dep = (0.9 + 0.0015 * x + 0.0007 * y + 0.0002 * rng.uniform(0, 1, (H, W))).astype(np.float32)
            a, n, d, _ = _guides(rng, W, H, "blocks", albedo=alb, normal=_unit_normals(rng, W, H, 0.05), depth=dep)
            col = _rgba(_smooth(rng, W, H, 3, 0.3, 2.0) * alb, rng)
            out.append(Case(f"atrous-joint-{W}x{H}-it{it}", "joint", "atrous", col, a, n, d, it, (0.6, 64.0, 0.2)))
            frames = 1 if W == 17 else 8
            out.append(Case(f"svgf-joint-{W}x{H}-it{it}-frames{frames}", "joint", "svgf", col, a, _with_moment(col, a, n, rng.uniform(0.1, 1.0, (H, W))), d, it,
                            (4.0, 128.0, 1.0), frames=frames))
    W, H = 17, 33
    a, n, d, _ = _guides(rng, W, H, "blocks")
    col = _rgba(_smooth(rng, W, H, 3, 0.5, 3.0), rng)
    out.append(Case("svgf-lum-two-iterations-17x33", "joint", "svgf", col, a, _with_moment(col, a, n, rng.uniform(0.05, 3.0, (H, W))), d, 2, (4.0, 0.0, OFF), frames=4))
    return out


def restate(case, dtype=np.float64):
    """The whole case through the restatements of tests/denoise_ref.py."""
    import denoise_ref as ref
    c = case
    if c.kind == "atrous":
        return ref._atrous_numpy(c.color, c.albedo, c.normal, c.iterations, c.sigmas[0], c.sigmas[1], c.sigmas[2], dtype)
    return ref._svgf_numpy(c.color, c.albedo, c.normal, c.depth, c.ref_frames, c.iterations, c.sigmas[0], c.sigmas[1], c.sigmas[2], dtype)


_EXPECTED = {}


def expected(case):
    """(float64 result (H, W, 4), bound on |device - result| (H, W, 3), CPU-side discrepancy): the discrepancy is max |float32 restatement -
    float64 restatement|, the conditioning of the case.  The bound comes from the arithmetic alone (tests/denoise_ref.py):
      structural   iterations * STRUCT_C * 2^-24 * max|input| (+ 2 roundings for SVGF's demodulation and re-modulation)
      numerical    the per-pixel first-order bound of the one iteration
      joint        16 x the discrepancy + the per-pixel bound of the first iteration"""
    import denoise_ref as ref
    if case.name in _EXPECTED:
        return _EXPECTED[case.name]
    c = case
    want = restate(c)
    disc = float(np.abs(restate(c, np.float32)[..., :3].astype(np.float64) - want[..., :3]).max())
    scale = float(np.abs(c.color[..., :3]).max())
    if c.tier == "structural":
        bound = np.full((c.H, c.W, 3), (c.iterations * ref.STRUCT_C + (0 if c.kind == "atrous" else 2)) * ref.U * scale)
    else:
        if c.kind == "atrous":
            _, bound = ref.atrous_iteration(c.color, c.albedo, c.normal, 1, c.sigmas[0], c.sigmas[1], c.sigmas[2], bound=True)
        else:
            _, bound, _ = ref.svgf_single(c.color, c.albedo, c.normal, c.depth, c.ref_frames, c.sigmas[0], c.sigmas[1], c.sigmas[2])
        if c.tier == "joint":
            bound = bound + 16.0 * disc
    _EXPECTED[case.name] = (want, bound, disc)
    return _EXPECTED[case.name]


def worst(got, want, bound):
    """(max error / bound, error there, bound there, (x, y, channel), distance of that pixel to the border)"""
    err = np.abs(got[..., :3].astype(np.float64) - want[..., :3])
    ratio = err / bound
    y, x, ch = np.unravel_index(np.argmax(ratio), ratio.shape)
    H, W = ratio.shape[:2]
    return float(ratio[y, x, ch]), float(err[y, x, ch]), float(bound[y, x, ch]), (int(x), int(y), int(ch)), int(min(x, y, W - 1 - x, H - 1 - y))


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = structural_cases() + numerical_cases() + joint_cases()
        assert len({c.name for c in _ALL}) == len(_ALL)
    return _ALL
