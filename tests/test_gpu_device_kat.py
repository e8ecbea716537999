"""Known-answer tests at FUNCTION level, on the device, of the shading and intersection code as the product compiles it.

tests/device_kat/libmi_pt_kat.so (built by build(); csrc/Makefile gives its object the variables of pt_kernels.o) wraps the unmodified device
headers in one-thread-per-case kernels.  The image tests see this code through an L2 norm over 15 k pixels; here every function is compared,
case by case, with the CPU oracle's hooks and with float64 closed forms at the inputs where kernels go wrong: grazing angles, roughness at its
floor, ior ratios next to 1 and next to total internal reflection, direction components 0 / -0 / denormal, node scales at both ends.

Bounds.  Exact class (divExact, sqrtExact, intersectTri, makeRaySetup, the node test against its numpy restatement): bit for bit.  Value class
(lobes, sky, lights, closed forms): MEASURED below holds, per group, the maximum and the 99.9th percentile of the relative difference to the
reference measured on the MI355X on the seeded random set; the asserted bound is max(2 x measured maximum, the bound the CPU test of the same
headers asserts) -- the factor 2 for the compiler rescheduling contractions between releases -- and never above CEILING = 1e-3, the whole
image's budget.  "Relative difference" is |device - reference| / (|reference| + floor) with floor = atol / rtol of the CPU test's allclose, so
`difference <= bound` is that allclose with rtol = bound.
"""
import ctypes as C
import os

import numpy as np
import pytest

import device_kat_lib as kat
import oracle_lib
from test_device_headers_on_host import LOBES, _mat
from test_oracle_pins import GOLD
from test_slab_offsets import SLAB_KINDS, _device_mask, _exact_mask, _slab_case, _spread
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

pytestmark = pytest.mark.gpu

F = C.c_float
F32 = np.float32
CEILING = 1e-3
EPS32 = float(np.finfo(np.float32).eps)

# group/key -> (maximum, 99.9th percentile) of the relative difference to the reference on the random set, measured on the MI355X
MEASURED = {
    "sample/anisotropic_metal": (3.240e-05, 2.548e-05),  # -> bound 1.0e-04
    "eval/anisotropic_metal": (6.850e-07, 6.096e-07),  # -> bound 2.0e-05
    "sample/clearcoat": (7.305e-04, 9.631e-05),  # -> bound 1.5e-03
    "eval/clearcoat": (7.691e-07, 7.307e-07),  # -> bound 2.0e-05
    "sample/dielectric": (2.893e-05, 2.148e-05),  # -> bound 1.0e-04
    "eval/dielectric": (6.859e-07, 6.322e-07),  # -> bound 2.0e-05
    "sample/diffuse": (1.005e-04, 7.084e-05),  # -> bound 2.0e-04
    "eval/diffuse": (0.000e+00, 0.000e+00),  # -> bound 2.0e-05
    "sample/diffuse_transmission": (6.250e-05, 4.195e-05),  # -> bound 1.3e-04
    "eval/diffuse_transmission": (7.751e-07, 6.574e-07),  # -> bound 2.0e-05
    "sample/dispersion": (9.856e-05, 3.274e-05),  # -> bound 2.0e-04
    "eval/dispersion": (2.077e-06, 1.546e-06),  # -> bound 2.0e-05
    "sample/dispersion_inside": (3.804e-05, 3.622e-05),  # -> bound 1.0e-04
    "eval/dispersion_inside": (1.302e-06, 1.160e-06),  # -> bound 2.0e-05
    "sample/everything": (5.409e-05, 3.842e-05),  # -> bound 1.1e-04
    "eval/everything": (3.084e-06, 2.015e-06),  # -> bound 2.0e-05
    "sample/iridescence_dielectric": (6.465e-05, 3.395e-05),  # -> bound 1.3e-04
    "eval/iridescence_dielectric": (1.206e-06, 9.981e-07),  # -> bound 2.0e-05
    "sample/iridescence_metal": (3.644e-05, 2.647e-05),  # -> bound 1.0e-04
    "eval/iridescence_metal": (1.103e-06, 8.489e-07),  # -> bound 2.0e-05
    "sample/metal": (9.356e-05, 7.929e-05),  # -> bound 1.9e-04
    "eval/metal": (7.102e-07, 5.740e-07),  # -> bound 2.0e-05
    "sample/metal_mix": (2.175e-04, 5.656e-05),  # -> bound 4.4e-04
    "eval/metal_mix": (7.132e-07, 6.464e-07),  # -> bound 2.0e-05
    "sample/retro_coat_sheen": (3.539e-05, 2.911e-05),  # -> bound 1.0e-04
    "eval/retro_coat_sheen": (2.329e-06, 1.897e-06),  # -> bound 2.0e-05
    "sample/retroreflection": (9.264e-05, 6.173e-05),  # -> bound 1.9e-04
    "eval/retroreflection": (6.449e-07, 5.480e-07),  # -> bound 2.0e-05
    "sample/sheen": (4.090e-05, 2.876e-05),  # -> bound 1.0e-04
    "eval/sheen": (3.494e-06, 1.544e-06),  # -> bound 2.0e-05
    "sample/specular_ext": (1.731e-04, 1.100e-04),  # -> bound 3.5e-04
    "eval/specular_ext": (8.382e-07, 7.431e-07),  # -> bound 2.0e-05
    "sample/transmission_inside": (6.015e-05, 3.857e-05),  # -> bound 1.2e-04
    "eval/transmission_inside": (2.720e-06, 1.392e-06),  # -> bound 2.0e-05
    "sample/transmission_thin": (1.717e-04, 6.299e-05),  # -> bound 3.4e-04
    "eval/transmission_thin": (6.029e-07, 5.558e-07),  # -> bound 2.0e-05
    "sample/transmission_volume": (4.135e-05, 3.006e-05),  # -> bound 1.0e-04
    "sky/eval": (1.522e-06, 1.181e-06),  # -> bound 3.0e-05
    "sky/pdf": (0.0, 0.0),  # -> bound 3.0e-05
    "sky/sample": (2.766e-05, 2.510e-05),  # -> bound 1.0e-04
    "lights": (4.149e-05, 1.718e-05),  # -> bound 8.3e-05
    "eval/transmission_volume": (1.562e-06, 1.140e-06),  # -> bound 2.0e-05
}


def _bound(key, host_bound):
    """max(2 x measured maximum, the host test's bound), capped by nothing: a measured maximum above CEILING / 2 fails _check_values' ceiling."""
    return max(2.0 * MEASURED.get(key, (0.0, 0.0))[0], host_bound)


def _rel(dev, ref, floor):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.abs(dev - ref) / (np.abs(ref) + floor)
    return np.where((dev == ref) | (np.isnan(dev) & np.isnan(ref)), 0.0, r)  # (equal infinities: inf - inf)


def _check_values(key, dev, ref, floor, host_bound):
    """Prints the measured figures (the source of MEASURED), then asserts the bound and the ceiling."""
    r = _rel(dev, ref, floor).reshape(len(dev), -1).max(axis=1) if len(dev) else np.zeros(1)
    worst, p999 = float(np.nanmax(r)) if not np.isnan(r).all() else float("nan"), float(np.nanpercentile(r, 99.9))
    bound = _bound(key, host_bound)
    print("KATMEASURE %-44s n %6d max %.3e p99.9 %.3e bound %.3e" % (key, len(dev), worst, p999, bound))
    assert not np.isnan(r).any(), (key, "NaN on one side only", int(np.isnan(r).argmax()))
    assert worst <= CEILING, (key, worst, int(r.argmax()), np.asarray(dev)[int(r.argmax())], np.asarray(ref)[int(r.argmax())])
    assert worst <= bound, (key, worst, bound, int(r.argmax()), np.asarray(dev)[int(r.argmax())], np.asarray(ref)[int(r.argmax())])
    return worst


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    """Bit for bit; NaN matches NaN (any payload)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def test_the_library_loads():
    """A missing library is a failure that names build(), not a skip."""
    kat.lib()


# =====================================================================================================================================
# a. exact class
# =====================================================================================================================================
def _mix(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def _operand_pairs(n, mode):
    """The operand pairs of tools/test_exact_math.hip: mode 0 = all bit patterns (denormals, infinities, NaNs), 1 = exponents within +-20 of 1."""
    i = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        ua = _mix(i * np.uint32(2) + np.uint32(1) + np.uint32((mode * 0x9e3779b9) & 0xffffffff))
        ub = _mix(i * np.uint32(2) + np.uint32(2) + np.uint32((mode * 0x85ebca6b) & 0xffffffff))
    if mode == 1:
        ua = (ua & np.uint32(0x807fffff)) | (((ua >> np.uint32(23)) % np.uint32(41) + np.uint32(107)) << np.uint32(23))
        ub = (ub & np.uint32(0x807fffff)) | (((ub >> np.uint32(23)) % np.uint32(41) + np.uint32(107)) << np.uint32(23))
    return ua.view(F32), ub.view(F32)


@pytest.mark.parametrize("ieee", [False, True], ids=["product_flags", "ieee_flags"])
@pytest.mark.parametrize("mode", [0, 1], ids=["all_bit_patterns", "ordinary_magnitudes"])
def test_div_exact_and_sqrt_exact_are_ieee_bit_for_bit(mode, ieee):
    """divExact(a, b) and sqrtExact(|a|) against numpy float32 a / b and sqrt (IEEE, correctly rounded) on 2^20 operand pairs, under both flag sets."""
    n = 1 << 20
    a, b = _operand_pairs(n, mode)
    special = ~np.isfinite(a) | (np.abs(a) < np.finfo(F32).tiny)
    assert mode == 1 or (special.sum() > 1000 and np.isnan(a).sum() > 100)  # the all-patterns mode does hold denormals, infinities and NaNs
    in3 = np.stack([a, b, np.zeros_like(a)], axis=1)
    with np.errstate(all="ignore"):
        q_ref, s_ref = (a / b).astype(F32), np.sqrt(np.abs(a)).astype(F32)
    q = kat.exact("div", in3, ieee)[:, 0]
    bad = ~_same_bits(q, q_ref)
    assert not bad.any(), ("divExact", int(bad.sum()), a[bad][:4], b[bad][:4], q[bad][:4], q_ref[bad][:4])
    in3[:, 0] = np.abs(a)
    s = kat.exact("sqrt", in3, ieee)[:, 0]
    bad = ~_same_bits(s, s_ref)
    assert not bad.any(), ("sqrtExact", int(bad.sum()), a[bad][:4], s[bad][:4], s_ref[bad][:4])


def test_libm_grade_helpers_do_not_depend_on_the_compile_options():
    """logExact / sinExact / cosExact / powExact / srgbOetf / normalizeExact: the same bits under both flag sets (the header's claim) and within 2 ulp
    of float64 (OCML documents 1 ulp for log, sin, cos and pow; one more for the rounding of the float64 reference and srgbOetf's fma)."""
    rng = np.random.default_rng(21)
    n = 200000
    x = np.concatenate([rng.uniform(0, 1, n // 2), 10.0 ** rng.uniform(-30, 30, n // 2)]).astype(F32)
    ang = np.concatenate([rng.uniform(-2 * np.pi, 2 * np.pi, n // 2), rng.uniform(-1e4, 1e4, n // 2)]).astype(F32)
    y = rng.uniform(-4, 4, n).astype(F32)
    z = np.zeros(n, F32)

    def ulps(got, ref64):
        ref = ref64.astype(F32)
        return np.abs(got.astype(np.float64) - ref64) / np.spacing(np.abs(ref)).astype(np.float64)

    for op, in3, ref in (("log", np.stack([x, z, z], 1), np.log(x.astype(np.float64))),
                         ("sin", np.stack([ang, z, z], 1), np.sin(ang.astype(np.float64))),
                         ("cos", np.stack([ang, z, z], 1), np.cos(ang.astype(np.float64))),
                         ("pow", np.stack([x[:n // 2], y[:n // 2], z[:n // 2]], 1), np.power(x[:n // 2].astype(np.float64), y[:n // 2].astype(np.float64))),
                         ("srgb", np.stack([x[:n // 2], z[:n // 2], z[:n // 2]], 1),
                          np.where(x[:n // 2] > F32(0.0031308), 1.055 * np.power(x[:n // 2].astype(np.float64), 1.0 / 2.4) - 0.055, x[:n // 2].astype(np.float64) * 12.92))):
        fast, ieee = kat.exact(op, in3, False)[:, 0], kat.exact(op, in3, True)[:, 0]
        assert _same_bits(fast, ieee).all(), op
        ok = np.isfinite(ref) & (np.abs(ref) > 1e-30) & (np.abs(ref) < 1e30)
        if op in ("sin", "cos"):
            ok &= np.abs(ref) > 1e-3  # (next to a zero of sin / cos an ulp of the RESULT is not the measure; the absolute error is)
            assert np.abs(fast.astype(np.float64) - ref).max() <= 2 * EPS32, op
        u = ulps(fast[ok], ref[ok])
        print("KATMEASURE exact/%-6s n %d max %.2f ulp" % (op, int(ok.sum()), float(u.max())))
        if op == "srgb":
            # srgbOetf = fma(p, 1.055, -0.055) with p = powExact(x, 1 / 2.4): the 2 ulp of p pass through the subtraction at their absolute size, which near the
            # 0.0031308 knee is 2.4 times as many ulp of the smaller result (measured there: 3.02); the fma adds half an ulp of the result, the reference's
            # rounding another half.  Stated per case; below the knee (x * 12.92) one rounding.
            xs = in3[:, 0].astype(np.float64)[ok]
            pw = np.power(xs, 1.0 / 2.4).astype(F32)
            allowed = np.where(xs > 0.0031308, 2.0 * 1.055 * np.spacing(pw).astype(np.float64) / np.spacing(np.abs(ref[ok].astype(F32))).astype(np.float64) + 1.0, 1.0)
            assert (u <= allowed).all(), (op, float((u / allowed).max()))
        else:
            assert u.max() <= 2.0, (op, float(u.max()))
    v = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-12, 12, (n, 1))).astype(F32)
    fast, ieee = kat.exact("normalize", v, False), kat.exact("normalize", v, True)
    assert _same_bits(fast, ieee).all()
    ref = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(fast - ref).max() <= 4 * EPS32  # dot (3 roundings), sqrt, reciprocal, product: 2.5 + 0.5 ulp of a component <= 1


def _tri_cases():
    """in15 rows (v0 e1 e2 org dir) and a tag per row."""
    rng = np.random.default_rng(31)
    rows, tags = [], []

    def add(tag, v0, e1, e2, org, d):
        rows.append(np.concatenate([v0, e1, e2, org, d]).astype(np.float64))
        tags.append(tag)

    def unit(v):
        return v / max(np.linalg.norm(v), 1e-300)

    for _ in range(6000):  # random triangles, rays aimed at and around them
        v0, e1, e2 = rng.uniform(-10, 10, 3), rng.normal(size=3) * 10.0 ** rng.uniform(-2, 1), rng.normal(size=3) * 10.0 ** rng.uniform(-2, 1)
        b = rng.uniform(-0.3, 1.3, 2)
        org = v0 + rng.normal(size=3) * 10.0 ** rng.uniform(-1, 2)
        add("random", v0, e1, e2, org, unit(v0 + b[0] * e1 + b[1] * e2 - org))
    for _ in range(4000):  # slivers: aspect up to 1e4, edges 2 mm .. 38 m (the sliver scenes)
        L = 10.0 ** rng.uniform(np.log10(0.002), np.log10(38.0))
        aspect = 10.0 ** rng.uniform(0, 4)
        a = unit(rng.normal(size=3))
        p = unit(np.cross(a, rng.normal(size=3)))
        v0, e1 = rng.uniform(-20, 20, 3), a * L
        e2 = a * L * rng.uniform(0.0, 1.0) + p * (L / aspect)
        b = rng.dirichlet((1, 1, 1))[:2] if rng.random() < 0.7 else rng.uniform(-0.2, 1.2, 2)
        org = v0 + rng.normal(size=3) * rng.uniform(0.5, 40.0)
        add("sliver", v0, e1, e2, org, unit(v0 + b[0] * e1 + b[1] * e2 - org))
    for _ in range(3000):  # through vertices and along edges
        v0, e1, e2 = rng.uniform(-5, 5, 3), rng.normal(size=3), rng.normal(size=3)
        v0, e1, e2 = v0.astype(F32).astype(np.float64), e1.astype(F32).astype(np.float64), e2.astype(F32).astype(np.float64)
        k = int(rng.integers(0, 6))
        t = rng.uniform(0, 1)
        target = [v0, v0 + e1, v0 + e2, v0 + t * e1, v0 + t * e2, v0 + e1 + t * (e2 - e1)][k]
        org = v0 + rng.normal(size=3) * rng.uniform(1, 10)
        add("vertex" if k < 3 else "edge", v0, e1, e2, org, unit(target - org))
    for _ in range(1000):  # det == 0 exactly: an axis-aligned triangle and a ray in its plane
        ax = int(rng.integers(0, 3))
        i, j = (ax + 1) % 3, (ax + 2) % 3
        e1, e2, d, v0, org = np.zeros(3), np.zeros(3), np.zeros(3), rng.uniform(-5, 5, 3), rng.uniform(-5, 5, 3)
        e1[i], e2[j] = rng.uniform(0.1, 3), rng.uniform(0.1, 3)
        d[i], d[j] = rng.normal(), rng.normal()
        org[ax] = v0[ax] if rng.random() < 0.5 else org[ax]
        add("det0", v0, e1, e2, org, unit(d))
    specials = [0.0, -0.0, 1e-38, -1e-38, 1e-45, -1e-45, float(np.nextafter(F32(1e-30), F32(0))), float(F32(1e-30)), float(np.nextafter(F32(1e-30), F32(1))),
                -float(np.nextafter(F32(1e-30), F32(0))), -float(F32(1e-30)), -float(np.nextafter(F32(1e-30), F32(1)))]
    for _ in range(3000):  # direction components 0, -0, denormal, on both sides of makeRaySetup's 1e-30
        v0, e1, e2 = rng.uniform(-5, 5, 3), rng.normal(size=3), rng.normal(size=3)
        b = rng.dirichlet((1, 1, 1))[:2]
        org = v0 + rng.normal(size=3) * rng.uniform(1, 10)
        d = unit(v0 + b[0] * e1 + b[1] * e2 - org)
        for a in rng.choice(3, size=int(rng.integers(1, 3)), replace=False):
            d[a] = specials[int(rng.integers(0, len(specials)))]
        add("special_dir", v0, e1, e2, org, d)
    with np.errstate(under="ignore"):
        return np.array(rows).astype(F32), np.array(tags)


def test_intersect_tri_matches_the_oracle_bit_for_bit_and_float64_on_well_conditioned_cases():
    O = oracle_lib.lib()
    in15, tags = _tri_cases()
    fast, ieee = kat.intersect_tri(in15, False), kat.intersect_tri(in15, True)
    ora = np.zeros_like(fast)
    o5 = (F * 5)()
    P = C.POINTER(F)
    for i, r in enumerate(in15):
        O.oracle_intersect_tri(r[0:9].ctypes.data_as(P), r[9:12].ctypes.data_as(P), r[12:15].ctypes.data_as(P), o5)
        ora[i] = o5[:]
    for name, got in (("product flags", fast), ("ieee flags", ieee)):
        bad = ~_same_bits(got, ora).all(axis=1)
        assert not bad.any(), (name, int(bad.sum()), tags[bad][:5], in15[bad][:2], got[bad][:2], ora[bad][:2])
    for t in np.unique(tags):
        print("KATCASES intersectTri %-12s n %5d hits %5d" % (t, int((tags == t).sum()), int(ora[tags == t, 0].sum())))
    assert ora[tags == "det0", 0].sum() == 0 and 0 < ora[:, 0].sum() < len(ora)
    # float64 Moeller-Trumbore.  Selected: cases whose float64 barycentrics lie at least 1e-4 from every edge (u = 0, v = 0, u + v = 1) AND whose float32
    # error estimate is a quarter of that margin at most.  The estimate: the numerator of u is a sum of products of a component each of tvec, dir, e2, that of
    # v of dir, tvec, e1, and det of e1, dir, e2; three fused dot / cross stages, the reciprocal and the product round each below 16 eps of those magnitudes,
    # and since u, v <= 1 the relative error of det counts once: 16 eps |dir| (|tvec| |e2| + |tvec| |e1| + |e1| |e2|) / |det|.  A cancelled det makes the
    # estimate large and deselects the case.
    v0, e1, e2, org, d = (in15[:, 3 * k:3 * k + 3].astype(np.float64) for k in range(5))
    pvec = np.cross(d, e2)
    det = (e1 * pvec).sum(1)
    with np.errstate(all="ignore"):
        tvec = org - v0
        u = (tvec * pvec).sum(1) / det
        v = (d * np.cross(tvec, e1)).sum(1) / det
        nt, nd, n1, n2 = (np.linalg.norm(x, axis=1) for x in (tvec, d, e1, e2))
        est = 16 * EPS32 * nd * (nt * n2 + nt * n1 + n1 * n2) / np.abs(det)
        margin = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(1.0 - u - v))
        sel = np.isfinite(u) & np.isfinite(v) & (margin >= 1e-4) & (est <= 2.5e-5)
    hit64 = (u >= 0) & (v >= 0) & (u + v <= 1)
    print("KATCASES intersectTri float64-selected %d of %d, hits %d" % (int(sel.sum()), len(sel), int((sel & hit64).sum())))
    assert sel.sum() > 1000 and (sel & hit64).sum() > 200 and (sel & ~hit64).sum() > 500  # (the generators do reach both outcomes: 1071 selected, 235 hits)
    assert ((fast[:, 0] > 0) == hit64)[sel].all()
    assert np.abs(fast[sel & hit64, 2] - u[sel & hit64]).max() <= 2.5e-5 and np.abs(fast[sel & hit64, 3] - v[sel & hit64]).max() <= 2.5e-5


def test_make_ray_setup_matches_the_oracle_bit_for_bit():
    """idir and ood: IEEE reciprocal of the direction (components below 1e-30 replaced by +-1e-30) and org * idir, under both flag sets; the oracle's walk
    divides 1 by the direction itself, so its hook is the reference wherever |dir| >= 1e-30 and numpy float32 everywhere."""
    O = oracle_lib.lib()
    in15, _ = _tri_cases()
    in6 = np.ascontiguousarray(in15[:, 9:15])
    fast, ieee = kat.ray_setup(in6, False), kat.ray_setup(in6, True)
    assert _same_bits(fast, ieee).all()
    d, org = in6[:, 3:6], in6[:, 0:3]
    eps = F32(1e-30)
    with np.errstate(all="ignore"):
        idir = (F32(1.0) / np.where(np.abs(d) < eps, np.copysign(eps, d), d).astype(F32)).astype(F32)
        ood = (org * idir).astype(F32)
    assert _same_bits(fast[:, 0:3], idir).all() and _same_bits(fast[:, 3:6], ood).all()
    assert np.isfinite(fast).all()
    small = np.abs(d) < eps
    assert small.sum() > 1000 and (np.abs(d) == eps).sum() > 100
    ora = np.zeros_like(fast)
    o6 = (F * 6)()
    P = C.POINTER(F)
    for i, r in enumerate(in6):
        O.oracle_ray_setup(r[0:3].ctypes.data_as(P), r[3:6].ctypes.data_as(P), o6)
        ora[i] = o6[:]
    big = ~small
    assert _same_bits(fast[:, 0:3], ora[:, 0:3])[big].all() and _same_bits(fast[:, 3:6], ora[:, 3:6])[big].all()


# =====================================================================================================================================
# b. the node test of the 8-wide walk
# =====================================================================================================================================
def _pack4(q):
    q = np.asarray(q, np.uint32)
    return [int(q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24)), int(q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24))]


def _pack_node(P, ebytes, qlo, qhi, imask, valid16):
    """The five uint4 of bvh8.hip's node layout (header comment of that file) and the 48 plane floats of DevScene::bvh8Planes."""
    w = [int(x) for x in np.asarray(P, F32).view(np.uint32)] + [int(ebytes[0]) | (int(ebytes[1]) << 8) | (int(ebytes[2]) << 16) | (int(imask) << 24)]
    w += [7, 11, int(valid16), 0]
    w += _pack4(qlo[0]) + _pack4(qlo[1]) + _pack4(qlo[2]) + _pack4(qhi[0]) + _pack4(qhi[1]) + _pack4(qhi[2])
    planes = np.concatenate([np.concatenate([qlo[a], qhi[a]]) for a in range(3)]).astype(F32)
    return w, planes


def _children_kinds(rng, qlo, qhi):
    """Leaf (one or two triangles) or inner for every non-empty slot: imask and valid16."""
    imask = valid = 0
    for sl in range(8):
        if qlo[0][sl] > qhi[0][sl]:
            continue
        k = int(rng.integers(0, 3))
        if k == 0:
            imask |= 1 << sl
        else:
            valid |= (3 if k == 2 else 1) << (2 * sl)
    return imask, valid


def _node_cases():
    """(P, ebytes, qlo, qhi, org, dir, tmax, tag).  The scale byte is e + 127 with e in -126 .. 126, i.e. 1 .. 253: quantiseAxis8 clamps the exponent
    (bvh_refit.h:84, returned at :114; the host collapse does the same at bvh8.hip:784 / :819); a node that is flat along an axis gets byte 1 and q = 0."""
    cases = []
    for kind in sorted(SLAB_KINDS, key=SLAB_KINDS.get):  # the generators of the CPU test, the same seeds
        rng = np.random.default_rng(SLAB_KINDS[kind])
        for _ in range(3000):
            P, s, qlo, qhi, org, d, tmax = _slab_case(rng, kind)
            cases.append((P, (np.log2(s) + 127).astype(int), qlo, qhi, org, d, tmax, kind))
    rng = np.random.default_rng(77)
    dir_specials = [0.0, -0.0, 1e-30, -1e-30, 1e-38, -1e-38]
    for n in range(9000):
        kind = ("outside", "inside", "graze")[n % 3]
        P, s, qlo, qhi, org, d, tmax = _slab_case(rng, kind)
        eb = (np.log2(s) + 127).astype(int)
        tag = ("on_plane", "tmax", "dir_special", "valid_count", "octant", "scale_small", "scale_large", "scale_large_q0", "flat_axis")[n % 9]
        if tag == "on_plane":  # origin exactly on a child plane (where P + q s is a float32, which it mostly is)
            a, c = int(rng.integers(0, 3)), int(rng.integers(0, 8))
            q = (qlo if rng.random() < 0.5 else qhi)[a][c]
            org[a] = F32(float(P[a]) + float(q) * float(s[a]))
        elif tag == "tmax":
            tmax = F32(0.0) if rng.random() < 0.5 else F32(np.inf)
        elif tag == "dir_special":
            for a in rng.choice(3, size=int(rng.integers(1, 3)), replace=False):
                d[a] = F32(dir_specials[int(rng.integers(0, len(dir_specials)))])
                if rng.random() < 0.5:
                    org[a] = F32(P[a] + s[a] * rng.uniform(0, 255))
        elif tag == "valid_count":  # 1 .. 8 valid children, the rest inverted
            keep = rng.permutation(8)[:int(rng.integers(1, 9))]
            for sl in range(8):
                if sl in keep and qlo[0][sl] > qhi[0][sl]:
                    qlo[:, sl] = rng.integers(0, 200, 3)
                    qhi[:, sl] = qlo[:, sl] + rng.integers(0, 55, 3)
                elif sl not in keep:
                    qlo[:, sl], qhi[:, sl] = 255, 0
        elif tag == "octant":
            d = (np.abs(d) * np.array([1 if (n // 9 >> a) & 1 else -1 for a in range(3)])).astype(F32)
        elif tag in ("scale_small", "flat_axis"):  # byte 1: s = 2^-126; the flat axis of a real node has every q = 0 and the ray anywhere
            a = int(rng.integers(0, 3))
            eb[a] = 1
            if tag == "flat_axis":
                live = qlo[0] <= qhi[0]
                qlo[a][live], qhi[a][live] = 0, 0
                if rng.random() < 0.5:
                    org[a] = P[a]
        else:  # byte 253: s = 2^126, A = s * idir overflows for |idir| > 4; with q == 0 the fma sees 0 * inf
            a = int(rng.integers(0, 3))
            eb[a] = 253
            org[a] = F32(rng.normal() * 10.0 ** rng.uniform(0, 37))
            if tag == "scale_large_q0":
                live = qlo[0] <= qhi[0]
                qlo[a][live] = 0
                d[a] = F32(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-6, -0.7))
        cases.append((P, eb, qlo, qhi, org, d, tmax, tag))
    return cases


def test_node_test_is_conservative_and_equals_the_numpy_restatement():
    cases = _node_cases()
    rng = np.random.default_rng(78)
    nodes, planes, rays, kinds = [], [], [], []
    for P, eb, qlo, qhi, org, d, tmax, tag in cases:
        imask, valid = _children_kinds(rng, qlo, qhi)
        w, pl = _pack_node(P, eb, qlo, qhi, imask, valid)
        nodes.append(w); planes.append(pl); rays.append(np.concatenate([org, d, [tmax]]).astype(F32)); kinds.append((imask, valid))
    out = kat.node_test(np.array(nodes, np.uint32), np.array(planes, F32), np.array(rays, F32))
    tags = np.array([c[7] for c in cases])
    missed, empty_hit, forms, leaf_bad, restated, checked, entered = [], [], [], [], [], {}, {}
    overflow = 0
    for i, (P, eb, qlo, qhi, org, d, tmax, tag) in enumerate(cases):
        s = np.ldexp(1.0, np.asarray(eb) - 127).astype(F32)
        hm, leaf, hmP = int(out[i, 0]), int(out[i, 1]), int(out[i, 2])
        dev = np.array([(hm >> c) & 1 for c in range(8)], bool)
        with np.errstate(all="ignore"):
            ex = _exact_mask(P, s, qlo, qhi, org, d, tmax)
            eps = F32(1e-30)
            dd = np.where(np.abs(d) < eps, np.copysign(eps, d), d).astype(F32)
            overflow += int(not np.isfinite(s * (F32(1.0) / dd)).all())
            # the device walks the direction makeRaySetup gives it: below 1e-30 that is +-1e-30, and the float64 test is asked about that ray
            if (np.abs(d) < eps).any():
                ex = _exact_mask(P, s, qlo, qhi, org, dd, tmax)
            rest = _device_mask(P, s, qlo, qhi, org, d, tmax)
        if (ex & ~dev).any():
            missed.append((i, tag, ex, dev))
        if (dev & (qlo[0] > qhi[0])).any():
            empty_hit.append((i, tag))
        if hm != hmP:
            forms.append((i, tag, hm, hmP))
        imask, valid = kinds[i]
        if leaf != (((_spread(hm) & valid) << 16) | valid):
            leaf_bad.append((i, tag, hm, valid, leaf))
        if (rest != dev).any():
            restated.append((i, tag, rest, dev))
        checked[tag] = checked.get(tag, 0) + int(ex.sum())
        entered[tag] = entered.get(tag, 0) + int(dev.sum())
    for t in sorted(checked):
        print("KATCASES node %-16s n %5d exact hits %6d device hits %6d" % (t, int((tags == t).sum()), checked[t], entered[t]))
    print("KATCASES node: A = s * idir overflows in %d cases" % overflow)
    assert overflow > 500
    assert sum(checked.values()) > 10000 and all(v > 0 for v in checked.values()), checked
    assert not missed, (len(missed), missed[:3], cases[missed[0][0]])  # 1. conservative, zero exceptions (both forms: 3. makes them one mask)
    assert not empty_hit, empty_hit[:5]  # 2. an empty slot is never reported hit
    assert not forms, (len(forms), forms[:5])  # 3. byte form == plane form
    assert not leaf_bad, leaf_bad[:5]  # 3. the leaf word is the doubling-and-valid16 rule
    assert not restated, (len(restated), restated[:3], cases[restated[0][0]])  # 4. the numpy restatement of the CPU tests IS the compiled function


# =====================================================================================================================================
# c. the lobes against the oracle
# =====================================================================================================================================
# The domain the product feeds bsdfSample / bsdfEvaluate (evaluateMaterial, pt_shading.h): roughness = max(r, MICROFACET_MIN_ROUGHNESS = 0.0014142)^2
# per axis (:19, :537); sheenRoughness >= the same floor (:658); clearcoatRoughness >= 0.001 (:613); metallic clamped to [0, 1] (:539); iridescence is
# switched off unless iridescenceThickness > 0 (:623) and the thickness is otherwise what the file says (the loader's defaults are 100 / 400 nm,
# gltf_scene.cpp:926-927, :986-987); dispersion is passed through unclamped (gltf_scene.cpp:1004, pt_shading.h:659) -- "the loader's maximum" does not
# exist, so 20 (the LOBES table's own maximum, an Abbe number of 1) and 100 stand in for it.
ROUGH_FLOOR = 0.0014142 ** 2
EVENT_ABSORB, EVENT_REFLECTION, EVENT_TRANSMISSION = 0, 8, 16


def _unit_np(rng, upper=False):
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    if upper:
        d[2] = abs(d[2])
    return d.astype(F32)


def _oracle_sample(O, m, k1, xi):
    out = (F * 8)()
    P = C.POINTER(F)
    res = np.zeros((len(m), 8), F32)
    for i in range(len(m)):
        O.oracle_bsdf_sample(m[i].ctypes.data_as(P), k1[i].ctypes.data_as(P), xi[i].ctypes.data_as(P), out)
        res[i] = out[:]
    return res


def _oracle_eval(O, m, k1, k2, xi):
    out = (F * 7)()
    P = C.POINTER(F)
    res = np.zeros((len(m), 4), F32)
    for i in range(len(m)):
        O.oracle_bsdf_eval(m[i].ctypes.data_as(P), k1[i].ctypes.data_as(P), k2[i].ctypes.data_as(P), xi[i].ctypes.data_as(P), out)
        o = np.array(out[:], F32)
        res[i] = [o[0] + o[3], o[1] + o[4], o[2] + o[5], o[6]]  # the device returns diffuse * occlusion + glossy in one vector (occlusion = 1)
    return res


def _random_set(lobe, n=1500):
    """The cases of test_bsdf_lobes_device_headers_match_oracle: same seed, same draws in the same order (k2 = a random direction or the oracle's sample)."""
    O = oracle_lib.lib()
    rng = np.random.default_rng(sum(map(ord, lobe)))
    m, k1, xi, k2 = np.zeros((n, 29), F32), np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    so = np.zeros((n, 8), F32)
    for i in range(n):
        m[i] = np.array(_mat(rng, **LOBES[lobe](rng))[:], F32)
        k1[i] = _unit_np(rng, upper=rng.random() < 0.9)
        xi[i] = rng.random(3).astype(F32)
        so[i] = _oracle_sample(O, m[i:i + 1], k1[i:i + 1], xi[i:i + 1])[0]
        k2[i] = _unit_np(rng) if rng.random() < 0.5 else so[i, 0:3]
    return m, k1, xi, k2, so


def _lobe_thresholds(O, m, vdotn):
    """The running weights findLobe compares xi.z with (lobes 5, 4, 3, 2, 1 in that order), from the oracle's computeLobeWeights."""
    w = (F * 6)()
    O.oracle_lobe_weights(m.ctypes.data_as(C.POINTER(F)), float(vdotn), w)
    acc, out = F32(0.0), []
    for l in (5, 4, 3, 2, 1):
        acc = F32(acc + F32(w[l]))
        if w[l] > 0.0 and 0.0 < acc < 1.0:
            out.append(acc)
    return out


def _edge_set(lobe):
    """One factor at a time on top of random materials of the lobe: (mat, k1, xi, tag, at_threshold)."""
    O = oracle_lib.lib()
    rng = np.random.default_rng(1000 + sum(map(ord, lobe)))
    one_minus = float(np.nextafter(F32(1.0), F32(0.0)))
    rows = []

    def base():
        d = LOBES[lobe](rng)
        return d, _unit_np(rng, upper=True), rng.random(3).astype(F32)

    def add(tag, over, k1, xi, thr=False):
        rows.append((np.array(_mat(np.random.default_rng(int(rng.integers(1 << 30))), **over)[:], F32), np.asarray(k1, F32), np.asarray(xi, F32), tag, thr))

    def graze(z, phi):
        s = np.sqrt(max(0.0, 1.0 - z * z))
        return np.array([s * np.cos(phi), s * np.sin(phi), z])

    for rep in range(6):
        for r in ((ROUGH_FLOOR, ROUGH_FLOOR), (1.0, 1.0), (1.0, 0.02), (0.02, 1.0), (ROUGH_FLOOR, 1.0)):
            d, k1, xi = base()
            add("roughness", dict(d, roughness=r, clearcoatRoughness=0.001 if "clearcoat" in d else 0.01, **({"sheenRoughness": 0.0014142} if "sheenRoughness" in d and rep % 2 else {})), k1, xi)
        for z in (1.0, 1e-2, 1e-4, 1e-6, -0.3, -1e-4):
            d, k1, xi = base()
            add("k1z", d, graze(z, rng.uniform(0, 2 * np.pi)), xi)
            add("k1z_rough_floor", dict(d, roughness=(ROUGH_FLOOR, ROUGH_FLOOR)), graze(z, rng.uniform(0, 2 * np.pi)), xi)
        for ratio, thr in ((1.0, True), (1.0 + 1e-6, True), (1.0 - 1e-6, True), (1.0 + 1e-3, False), (1.0 - 1e-3, False)):
            d, k1, xi = base()
            i1 = d.get("ior1", 1.0)
            add("ior_ratio", dict(d, ior1=i1, ior2=float(F32(i1 * ratio))), k1, xi, thr)
        if LOBES[lobe](rng).get("ior1", 1.0) > 1.0:  # the inside lobes: k1.z at the critical angle of the macro-surface +- 1 ulp, smooth and rough
            for _ in range(3):
                d, k1, xi = base()
                zc = F32(np.sqrt(1.0 - (d["ior2"] / d["ior1"]) ** 2))
                for z in (np.nextafter(zc, F32(0)), zc, np.nextafter(zc, F32(1))):
                    add("critical_angle", dict(d, roughness=(ROUGH_FLOOR, ROUGH_FLOOR)), graze(float(z), 0.3), xi, True)
                    add("critical_angle", d, graze(float(z), 0.3), xi, True)
        for key in ("metallic", "transmission", "clearcoat", "iridescence"):
            for val in (0.0, 1.0):
                d, k1, xi = base()
                add(key, dict(d, **{key: val}), k1, xi)
        for th in (1e-3, 100.0, 400.0, 1200.0):
            d, k1, xi = base()
            add("iridescenceThickness", dict(d, iridescence=d.get("iridescence", 0.7), iridescenceThickness=th), k1, xi)
        for disp in (0.0, 20.0, 100.0):
            d, k1, xi = base()
            add("dispersion", dict(d, dispersion=disp), k1, xi)
        for comp in range(3):
            for val in (0.0, one_minus):
                d, k1, xi = base()
                xi[comp] = val
                add("xi_end", d, k1, xi, True)  # (xi.x next to 1 is the rim of the sampling disc, where h.z == 0 decides absorption: a threshold)
        d, k1, xi = base()
        add("xi_end", d, k1, [0.0, 0.0, 0.0], True)
        add("xi_end", d, k1, [one_minus] * 3, True)
        d, k1, xi = base()  # both sides of each lobe-pick threshold
        m = np.array(_mat(np.random.default_rng(5), **d)[:], F32)
        for t in _lobe_thresholds(O, m, k1[2]):
            for z in (np.nextafter(t, F32(0)), t, np.nextafter(t, F32(1))):
                rows.append((m, k1, np.array([xi[0], xi[1], z], F32), "lobe_threshold", True))
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]), np.array([r[3] for r in rows]),
            np.array([r[4] for r in rows]))


# |k2| - 1 of the ORACLE's own samples, measured on the CPU over the random and the edge sets of all 19 lobes: 5.8e-7 (the reflected direction
# 2 (k1.h) h - k1 is not renormalised: a handful of float32 products and sums); the device may be 4 x that far off for its approximate sin / cos
ORACLE_K2_UNIT = 5.8e-7
K2_UNIT_BOUND = 4 * ORACLE_K2_UNIT


def _check_properties(tag, m, k1, xi, s):
    """Device alone, no measured tolerance: finite, non-negative, absorbed => zero, k2 on its side and of unit length."""
    ev = s[:, 7].astype(int)
    assert np.isfinite(s).all(), (tag, "non-finite", m[~np.isfinite(s).all(1)][:1], k1[~np.isfinite(s).all(1)][:1], xi[~np.isfinite(s).all(1)][:1], s[~np.isfinite(s).all(1)][:1])
    assert (s[:, 6] >= 0).all() and (s[:, 3:6] >= 0).all(), (tag, "negative pdf or weight")
    ab = ev == EVENT_ABSORB
    assert (s[ab, 3:7] == 0).all(), (tag, "an absorbed sample carries weight or pdf")
    live = ~ab
    refl, trans = live & ((ev & EVENT_REFLECTION) != 0), live & ((ev & EVENT_TRANSMISSION) != 0)
    assert (refl ^ trans)[live].all(), (tag, "event type is neither reflection nor transmission", np.unique(ev))
    assert (s[refl, 2] > 0).all() and (s[trans, 2] < 0).all(), (tag, "k2 on the wrong side")
    if live.any():
        dev_unit = np.abs(np.linalg.norm(s[live, 0:3].astype(np.float64), axis=1) - 1.0)
        print("KATMEASURE k2unit/%-37s n %6d max %.3e bound %.3e" % (tag, int(live.sum()), float(dev_unit.max()), K2_UNIT_BOUND))
        assert dev_unit.max() <= K2_UNIT_BOUND, (tag, float(dev_unit.max()), m[live][dev_unit.argmax()], k1[live][dev_unit.argmax()], xi[live][dev_unit.argmax()])


def _consistency(s, e):
    """Relative difference of the evaluated pdf and of bsdf / pdf to what the sampler returned, per case (inf where the evaluated pdf is not positive)."""
    pdf_s, w_s, pdf_e, b_e = s[:, 6].astype(np.float64), s[:, 3:6].astype(np.float64), e[:, 3].astype(np.float64), e[:, 0:3].astype(np.float64)
    with np.errstate(all="ignore"):
        r_pdf = np.abs(pdf_e - pdf_s) / np.abs(pdf_s)
        r_w = (np.abs(b_e / pdf_e[:, None] - w_s) / (np.abs(w_s) + 1e-5 / 3e-3)).max(axis=1)
    bad = ~(pdf_e > 0) | ~np.isfinite(r_pdf) | ~np.isfinite(r_w)
    return np.where(bad, np.inf, r_pdf), np.where(bad, np.inf, r_w)


def _check_consistency(tag, m, k1, xi, s, so):
    """For the directions the device samples, its bsdfEvaluate returns the same pdf within 2e-3 and bsdf / pdf == bsdf_over_pdf within 3e-3, the bounds of
    test_bsdf_sample_eval_consistency (which skips pdf <= 0 the same way).  Asserted on the cases where the property is a statement about the code and not
    about float32: evaluating at a SAMPLED direction recomputes the half vector from a rounded k2, an angle error of 1e-7 that a GGX lobe of roughness alpha
    amplifies by 2 / alpha (alpha goes down to 2e-6 here) and index-matched refraction by 1 / |ior2 / ior1 - 1|.  The selection comes from the reference's own
    error: a case counts where the ORACLE's sample and evaluation (IEEE, libm) agree within a quarter of the bounds, also after a 1e-6 nudge of k2."""
    O = oracle_lib.lib()
    live = (s[:, 7] != 0) & (so[:, 7] == s[:, 7])
    if not live.any():
        return 0
    m, k1, xi, s, so = m[live], k1[live], xi[live], s[live], so[live]
    e = kat.bsdf_eval(m, k1, np.ascontiguousarray(s[:, 0:3]), xi)
    assert np.isfinite(e).all() and (e >= 0).all(), (tag, "evaluation at a sampled direction is negative or not finite", m[~np.isfinite(e).all(1)][:1], k1[~np.isfinite(e).all(1)][:1],
                                                      xi[~np.isfinite(e).all(1)][:1], s[~np.isfinite(e).all(1)][:1])
    o_pdf, o_w = _consistency(so, _oracle_eval(O, m, k1, np.ascontiguousarray(so[:, 0:3]), xi))
    well = (o_pdf <= 2e-3 / 4) & (o_w <= 3e-3 / 4)
    # ... and where it stays so when the direction moves by what separates two float32 samplers, 1e-6 (a few ulp of k2: the device draws the azimuth with
    # v_sin / v_cos, 1.3e-7 absolute): the oracle's evaluation at k2 +- 1e-6 along two tangents must not move by more than the same quarter
    k2o = so[:, 0:3].astype(np.float64)
    t1 = np.cross(k2o, np.where(np.abs(k2o[:, 2:3]) < 0.9, [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0]]))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(k2o, t1)
    for t in (t1, -t1, t2, -t2):
        kp = k2o + 1e-6 * t
        kp /= np.linalg.norm(kp, axis=1, keepdims=True)
        p_pdf, p_w = _consistency(so, _oracle_eval(O, m, k1, kp.astype(F32), xi))
        well &= (p_pdf <= 2e-3 / 4) & (p_w <= 3e-3 / 4)
    r_pdf, r_w = _consistency(s, e)
    print("KATMEASURE consistency/%-32s n %6d of %6d sampled; pdf %.3e weight %.3e" % (tag, int(well.sum()), len(well), float(r_pdf[well].max()) if well.any() else 0.0,
                                                                                       float(r_w[well].max()) if well.any() else 0.0))
    if well.any():
        i = int(np.where(well, np.maximum(r_pdf / 2e-3, r_w / 3e-3), 0).argmax())
        assert r_pdf[well].max() <= 2e-3 and r_w[well].max() <= 3e-3, (tag, float(r_pdf[i]), float(r_w[i]), m[i], k1[i], xi[i], s[i], e[i])
    return int(well.sum())


@pytest.mark.parametrize("lobe", sorted(LOBES))
def test_lobes_on_the_device_match_the_oracle(lobe):
    m, k1, xi, k2, so = _random_set(lobe)
    sd = kat.bsdf_sample(m, k1, xi)
    ed = kat.bsdf_eval(m, k1, k2, xi)
    eo = _oracle_eval(oracle_lib.lib(), m, k1, k2, xi)
    # event type: at most 1e-3 of the cases may differ (a lobe pick or TIR decision that flips on the last bit); counted, printed, left out of the values
    differ = sd[:, 7] != so[:, 7]
    print("KATCASES lobe %-24s n %d event-type exceptions %d" % (lobe, len(m), int(differ.sum())))
    for i in np.nonzero(differ)[0][:4]:
        print("   exception: mat", m[i].tolist(), "k1", k1[i].tolist(), "xi", xi[i].tolist(), "device", sd[i].tolist(), "oracle", so[i].tolist())
    assert differ.sum() <= 1e-3 * len(m), (lobe, int(differ.sum()))
    same = ~differ & (so[:, 7] != 0)
    assert same.sum() > 100 and (eo[:, 3] > 0).sum() > 100
    _check_properties("random/" + lobe, m, k1, xi, sd)
    assert (ed >= 0).all() and np.isfinite(ed).all()
    assert _check_consistency("random/" + lobe, m, k1, xi, sd, so) > 0.6 * same.sum()  # (the selection keeps the bulk of every lobe)
    failures = []
    for key, dev, ref, floor, host in (("sample/" + lobe, sd[same, 0:7], so[same, 0:7], 1e-6 / 1e-4, 1e-4), ("eval/" + lobe, ed, eo, 1e-7 / 2e-5, 2e-5)):
        try:
            _check_values(key, dev, ref, floor, host)
        except AssertionError as e:  # (both figures are printed before either fails)
            failures.append(e)
    assert not failures, failures


@pytest.mark.parametrize("lobe", sorted(LOBES))
def test_lobes_on_the_device_keep_their_properties_at_the_edges_of_the_domain(lobe):
    m, k1, xi, tags, thr = _edge_set(lobe)
    sd = kat.bsdf_sample(m, k1, xi)
    so = _oracle_sample(oracle_lib.lib(), m, k1, xi)
    for t in np.unique(tags):
        sel = tags == t
        print("KATCASES edge %-24s %-22s n %4d absorbed %4d event-type differences to the oracle %d" % (lobe, t, int(sel.sum()), int((sd[sel, 7] == 0).sum()),
                                                                                                   int((sd[sel, 7] != so[sel, 7]).sum())))
    _check_properties("edge/" + lobe, m, k1, xi, sd)
    _check_consistency("edge/" + lobe, m, k1, xi, sd, so)
    # away from the cases that sit on a threshold on purpose, the event type is the oracle's
    differ = (sd[:, 7] != so[:, 7]) & ~thr
    assert not differ.any(), (lobe, int(differ.sum()), tags[differ][:4], m[differ][:1], k1[differ][:1], xi[differ][:1], sd[differ][:1], so[differ][:1])
    # the simple-material sampler on the same inputs: same properties
    ss = kat.bsdf_sample(m, k1, xi, simple=True)
    _check_properties("edge_simple/" + lobe, m, k1, xi, ss)


FURNACE = [dict(baseColor=(1, 1, 1), metallic=0.0, specular=0.0), dict(baseColor=(1, 1, 1), metallic=1.0, roughness=(0.3, 0.3)),
           dict(baseColor=(1, 1, 1), metallic=0.0, roughness=(0.2, 0.2)), dict(baseColor=(1, 1, 1), transmission=1.0, roughness=(0.1, 0.1), thickness=1.0),
           dict(baseColor=(1, 1, 1), clearcoat=1.0, roughness=(0.5, 0.5)), dict(baseColor=(1, 1, 1), sheenColor=(1, 1, 1), sheenRoughness=0.5)]


@pytest.mark.parametrize("which", range(len(FURNACE)))
def test_white_furnace_on_the_device(which):
    """test_bsdf_white_furnace's six materials, view and bounds, sampled by the device: with every colour 1 the weight never exceeds 1 + 1e-4."""
    import test_oracle_kat
    m1 = np.array(test_oracle_kat._mat(**FURNACE[which])[:], F32)
    n = 4000
    theta = np.radians(50.0)
    xi = np.random.default_rng(1).random((n, 3)).astype(F32)
    s = kat.bsdf_sample(np.tile(m1, (n, 1)), np.tile(np.array([np.sin(theta), 0.0, np.cos(theta)], F32), (n, 1)), xi)
    w = s[:, 3:6]
    assert np.isfinite(s).all()
    print("KATMEASURE furnace/%d max %.7f mean %.5f" % (which, float(w.max()), float(w.mean())))
    assert w.max() <= 1.0 + 1e-4
    assert 0.5 < w.mean() <= 1.0 + 1e-6


def test_evaluated_pdf_integrates_to_one_on_the_device():
    """test_bsdf_pdf_normalised on the device: the Monte-Carlo integral of the evaluated pdf over the sphere is 1 minus the absorbed share."""
    import test_oracle_kat
    rng = np.random.default_rng(7)
    n = 20000
    m1 = np.array(test_oracle_kat._mat(baseColor=(0.9, 0.9, 0.9), metallic=0.0, roughness=(0.3, 0.3))[:], F32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = kat.bsdf_eval(np.tile(m1, (n, 1)), np.tile(np.array([0.5, 0.0, 0.8660254], F32), (n, 1)), d.astype(F32), rng.random((n, 3)).astype(F32))
    integral = float(e[:, 3].astype(np.float64).mean() * 4 * np.pi)
    print("KATMEASURE pdf integral %.4f" % integral)
    assert 0.85 < integral < 1.05


# =====================================================================================================================================
# d. closed forms against float64 (tests/golden/pins_closed_forms.json; the tolerances test_oracle_pins.py asserts for the oracle)
# =====================================================================================================================================
def _approx(key, got, want, rel, abs_=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = np.maximum(rel * np.abs(want), abs_)
    ratio = np.abs(got - want) / tol
    print("KATMEASURE closed/%-24s n %5d worst |err| / tolerance %.3f (rel %.1e abs %.1e)" % (key, got.size, float(ratio.max()), rel, abs_))
    assert ratio.max() <= 1.0, (key, float(ratio.max()), int(ratio.argmax()))


def test_fresnel_terms_on_the_device_match_the_closed_forms():
    g = GOLD["fresnel_dielectric"]
    _approx("fresnel_dielectric", kat.blocks("ior_fresnel", [[e["eta"], e["cos"]] for e in g])[:, 0], [e["R"] for e in g], 2e-5, 2e-7)
    assert kat.blocks("ior_fresnel", [[1.5, 1.0]])[0, 0] == pytest.approx(0.04, rel=1e-6)
    g = GOLD["fresnel_schlick"]
    _approx("fresnel_schlick", kat.blocks("schlick", [[e["ior"], e["cos"]] for e in g])[:, 0], [e["R"] for e in g], 2e-5, 1e-7)
    g = GOLD["fresnel_conductor"]
    out = kat.blocks("conductor", [[e["n_a"], e["n_b"], e["k_b"], e["cos"]] for e in g])
    _approx("fresnel_conductor_s", out[:, 0], [e["Rs"] for e in g], 5e-5, 1e-6)
    _approx("fresnel_conductor_p", out[:, 1], [e["Rp"] for e in g], 5e-5, 1e-6)
    # fresnel_dielectric (the amplitude pair of the thin-film term) against Fresnel's equations in float64, Snell's angle from float64 too
    rng = np.random.default_rng(41)
    na, nb, ca = rng.uniform(1.0, 2.0, 2000), rng.uniform(1.0, 2.5, 2000), rng.uniform(0.02, 1.0, 2000)
    sb2 = (na / nb) ** 2 * (1 - ca * ca)
    ok = sb2 < 0.98
    na, nb, ca, cb = na[ok], nb[ok], ca[ok], np.sqrt(1 - sb2[ok])
    na, nb, ca, cb = (x.astype(F32).astype(np.float64) for x in (na, nb, ca, cb))
    out = kat.blocks("fresnel_dielectric", np.stack([na, nb, ca, cb], 1))
    _approx("fresnel_dielectric_s", out[:, 0], ((na * ca - nb * cb) / (na * ca + nb * cb)) ** 2, 5e-5, 1e-7)
    _approx("fresnel_dielectric_p", out[:, 1], ((nb * ca - na * cb) / (nb * ca + na * cb)) ** 2, 5e-5, 1e-7)


def test_total_internal_reflection_threshold_on_the_device():
    """isTIR: total internal reflection iff sin(theta) > ior2 / ior1, i.e. (ior1 / ior2)^2 (1 - kh^2) > 1 -- STRICTLY: at the critical angle itself the refracted
    direction still exists (grazing).  Float64 on seeded cases at least 1e-5 from the threshold (the float32 expression carries five roundings, 3e-7), and the
    cases where the threshold is met exactly in any arithmetic: index-matched media (ior1 == ior2 a power of two: the reciprocal is exact) at kh = 0."""
    rng = np.random.default_rng(43)
    n = 20000
    i1, i2, kh = rng.uniform(1.0, 2.5, n).astype(F32), rng.uniform(1.0, 2.5, n).astype(F32), rng.uniform(0.0, 1.0, n).astype(F32)
    x = (i1.astype(np.float64) / i2) ** 2 * (1.0 - kh.astype(np.float64) ** 2)
    far = np.abs(x - 1.0) >= 1e-5
    got = kat.blocks("is_tir", np.stack([i1, i2, kh], 1))[:, 0]
    assert far.sum() > 0.99 * n and 0.2 * n < (x > 1).sum() < 0.8 * n
    assert ((got > 0) == (x > 1))[far].all()
    exact = kat.blocks("is_tir", [[1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [4.0, 4.0, 0.0], [0.5, 0.5, 0.0], [1.0, 1.0, -0.0]])[:, 0]
    assert (exact == 0).all(), exact
    assert (kat.blocks("is_tir", [[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [2.0, 1.0, 0.875], [2.0, 1.0, 0.75]])[:, 0] == [1, 0, 0, 1]).all()  # 4 (1 - 0.765625) = 0.9375, 4 (1 - 0.5625) = 1.75


def test_thin_film_on_the_device_matches_the_airy_formula():
    g = GOLD["thin_film"]
    rgb = kat.blocks("thin_film", [[e["thickness"], e["coating_ior"], e["base_ior"], e["incoming_ior"], e["cos"]] for e in g])[:, 0:3]
    worst, exact_cases = 0.0, 0
    for e, c in zip(g, rgb):
        err = float(np.abs(c - np.array(e["rgb"])).max())
        if e["p_sign_band"]:
            assert err < 0.12, (e, c)
        elif e["near_brewster"]:
            assert err < 5e-3, (e, c)
        else:
            worst = max(worst, err)
            exact_cases += 1
            assert np.allclose(c, e["rgb"], rtol=3e-4, atol=3e-5), (e, c)
    print("KATMEASURE closed/thin_film exact cases %d worst %.3e (bound 3e-4)" % (exact_cases, worst))
    assert worst < 3e-4 and exact_cases >= 40
    assert np.allclose(kat.blocks("thin_film", [[0.0, 1.3, 1.5, 1.0, 1.0]])[0, 0:3], 0.04, rtol=1e-3)


def test_ggx_distribution_masking_and_vndf_on_the_device():
    import test_oracle_kat  # noqa: F401
    g = GOLD["ggx"]
    inv = lambda e: [float(F32(1.0) / F32(e["ax"])), float(F32(1.0) / F32(e["ay"]))]
    _approx("ggx_D_cos", kat.blocks("ggx_ndf", [inv(e) + list(e["h"]) for e in g])[:, 0], [e["D_cos"] for e in g], 3e-5)
    _approx("ggx_G1", kat.blocks("ggx_g1", [[e["ax"], e["ay"]] + list(e["v"]) for e in g])[:, 0], [e["G1_v"] for e in g], 3e-5)
    # a view direction with roughness components that differ: swapping them must show (an isotropic table would not notice)
    assert any(abs(e["ax"] - e["ay"]) > 0.1 and abs(abs(e["v"][0]) - abs(e["v"][1])) > 0.1 for e in g)
    mat = np.zeros(29, F32)
    mat[0:3] = 1.0; mat[5] = 1.0; mat[6], mat[7], mat[8] = 1.0, 1.5, 1.0; mat[9:12] = 1.0; mat[15] = 0.01; mat[21], mat[22] = 1.5, 100.0; mat[24:27] = 1.0
    sel = [e for e in g if "l" in e and e["l"][2] > 1e-3]
    ms = np.tile(mat, (len(sel), 1))
    ms[:, 3], ms[:, 4] = [e["ax"] for e in sel], [e["ay"] for e in sel]
    ev = kat.bsdf_eval(ms, np.array([e["v"] for e in sel], F32), np.array([e["l"] for e in sel], F32), np.tile(np.array([0.3, 0.6, 0.5], F32), (len(sel), 1)))
    assert len(sel) > 20
    _approx("ggx_vndf_reflected_pdf", ev[:, 3], [e["vndf_reflected_pdf"] for e in sel], 1e-4)
    _approx("ggx_G1_l", ev[:, 0].astype(np.float64) / ev[:, 3], [e["G1_l"] for e in sel], 1e-4)
    # Heitz 2018: sample means of three test functions against quadrature over D_v (test_ggx_vndf_samples_follow_the_visible_normal_distribution)
    rng = np.random.default_rng(5)
    for ax, ay, v in ((0.4, 0.4, (0.6, 0.0, 0.8)), (0.7, 0.2, (0.5, 0.5, 0.7071)), (0.15, 0.5, (0.9, -0.3, 0.316))):
        v = np.array(v) / np.linalg.norm(v)
        n = 60000
        uv = rng.random((n, 2))
        hs = kat.blocks("ggx_vndf", np.concatenate([np.tile([ax, ay, *v], (n, 1)), uv], 1))[:, 0:3].astype(np.float64)
        assert np.abs(np.linalg.norm(hs, axis=1) - 1).max() < 1e-5
        th, ph = np.meshgrid((np.arange(400) + 0.5) / 400 * (np.pi / 2), (np.arange(800) + 0.5) / 800 * 2 * np.pi, indexing="ij")
        H = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1)
        D = 1.0 / (np.pi * ax * ay * ((H[..., 0] / ax) ** 2 + (H[..., 1] / ay) ** 2 + H[..., 2] ** 2) ** 2)
        lam = 0.5 * (-1 + np.sqrt(1 + ((ax * v[0]) ** 2 + (ay * v[1]) ** 2) / v[2] ** 2))
        w = np.maximum(H @ v, 0) * D / (1 + lam) / v[2] * np.sin(th) * (np.pi / 2 / 400) * (2 * np.pi / 800)
        for fn in (lambda X: X[..., 2], lambda X: X[..., 0], lambda X: X[..., 1] ** 2):
            assert fn(hs).mean() == pytest.approx((fn(H) * w).sum() / w.sum(), abs=6e-3)


def test_sheen_density_and_henyey_greenstein_on_the_device():
    g = GOLD["sheen"]
    _approx("sheen_pdf_h", kat.blocks("sheen_ndf", [[e["n"], e["cos_h"]] for e in g])[:, 0], [e["pdf_h"] for e in g], 5e-5, 1e-30)
    g = [e for e in GOLD["henyey_greenstein"] if abs(1 + e["g"] ** 2 - 2 * e["g"] * e["cos"]) >= 1e-4]
    pdf = kat.blocks("hg_pdf", [[e["cos"], e["g"]] for e in g])[:, 0]
    hi = np.array([abs(e["g"]) > 0.9 for e in g])
    _approx("hg_pdf", pdf[~hi], [e["pdf"] for e, h in zip(g, hi) if not h], 3e-5)
    _approx("hg_pdf_g>0.9", pdf[hi], [e["pdf"] for e, h in zip(g, hi) if h], 2e-4)
    rng = np.random.default_rng(2)
    wi = np.array([0.3, -0.5, 0.81])
    wi /= np.linalg.norm(wi)
    for gg in (-0.6, 0.0, 0.35, 0.85):
        n = 20000
        uv = rng.random((n, 2))
        wo = kat.blocks("hg_sample", np.concatenate([uv, np.tile([gg, *wi], (n, 1))], 1))[:, 0:3].astype(np.float64)
        assert np.abs(np.linalg.norm(wo, axis=1) - 1).max() <= 1e-5
        assert (wo @ wi).mean() == pytest.approx(gg, abs=0.012)


# =====================================================================================================================================
# e. sky and lights against the oracle
# =====================================================================================================================================
def _sky_trials():
    rng = np.random.default_rng(3)
    for trial in range(6):
        sky = ptmod.default_sky()
        if trial:
            sky.haze, sky.redblueshift, sky.saturation = rng.uniform(0, 8), rng.uniform(-0.5, 0.5), rng.uniform(0.2, 1.5)
            sky.horizonHeight, sky.horizonBlur, sky.sunDiskScale, sky.sunGlowIntensity = rng.uniform(-0.2, 0.2), rng.uniform(0.05, 1), rng.uniform(0.5, 4), rng.uniform(0, 2)
            d = rng.normal(size=3); d[1] = abs(d[1]) + 0.05; d /= np.linalg.norm(d)
            sky.sunDirection[:] = d.tolist()
            sky.yIsUp = int(trial % 2)
            if not sky.yIsUp:
                sky.sunDirection[:] = [d[0], d[2], d[1]]
        dirs = np.array([_unit_np(rng) for _ in range(400)])
        uv = rng.random((400, 2)).astype(F32)
        # edges: the horizon +- 1 ulp of the up component, the sun direction exactly, u, v at 0 and at the largest float below 1
        up = 1 if sky.yIsUp else 2
        hz = F32(sky.horizonHeight * 0.1)
        edge_dirs = []
        for z in (np.nextafter(hz, F32(-1)), hz, np.nextafter(hz, F32(1)), F32(0.0)):
            phi = rng.uniform(0, 2 * np.pi)
            s = np.sqrt(1 - float(z) ** 2)
            e = np.zeros(3, F32)
            e[up], e[(up + 1) % 3], e[(up + 2) % 3] = z, F32(s * np.cos(phi)), F32(s * np.sin(phi))
            edge_dirs.append(e)
        sun = np.array(sky.sunDirection[:], np.float64)
        edge_dirs.append((sun / np.linalg.norm(sun)).astype(F32))
        one_minus = np.nextafter(F32(1), F32(0))
        edge_uv = [(a, b) for a in (F32(0), one_minus, F32(0.5)) for b in (F32(0), one_minus)]
        n = max(len(edge_dirs), len(edge_uv))
        ed = np.array([edge_dirs[i % len(edge_dirs)] for i in range(n)], F32)
        eu = np.array([edge_uv[i % len(edge_uv)] for i in range(n)], F32)
        yield trial, sky, dirs, uv, ed, eu


def _oracle_sky(O, sky, dirs, uv):
    out = np.zeros((len(dirs), 11), F32)
    a, sa = (F * 3)(), (F * 7)()
    for i in range(len(dirs)):
        dr = (F * 3)(*dirs[i])
        O.oracle_sky_eval(C.byref(sky), dr, a)
        out[i, 0:3] = a[:]
        out[i, 3] = O.oracle_sky_pdf(C.byref(sky), dr)
        O.oracle_sky_sample(C.byref(sky), float(uv[i, 0]), float(uv[i, 1]), sa)
        out[i, 4:11] = sa[:]
    return out


def test_sky_on_the_device_matches_the_oracle():
    O = oracle_lib.lib()
    dev_all, ora_all = [], []
    for trial, sky, dirs, uv, ed, eu in _sky_trials():
        dev = kat.sky(sky, np.concatenate([dirs, uv], 1))
        ora = _oracle_sky(O, sky, dirs, uv)
        dev_all.append(dev); ora_all.append(ora)
        assert np.isfinite(dev).all() and (dev[:, 3] >= 0).all() and (dev[:, 7] >= 0).all() and (dev[:, [0, 1, 2, 8, 9, 10]] >= 0).all()
        edge = kat.sky(sky, np.concatenate([ed, eu], 1))
        assert np.isfinite(edge).all() and (edge[:, 3] >= 0).all() and (edge[:, 7] >= 0).all() and (edge[:, [0, 1, 2, 8, 9, 10]] >= 0).all(), (trial, edge)
        assert np.abs(np.linalg.norm(edge[:, 4:7].astype(np.float64), axis=1) - 1).max() <= K2_UNIT_BOUND * 4
        # at the edges the oracle is the reference too, apart from the two directions that sit on the horizon test within an ulp
        oe = _oracle_sky(O, sky, ed, eu)
        keep = np.ones(len(ed), bool)
        keep[[i for i in range(len(ed)) if i % 5 in (0, 1, 2)]] = False
        assert np.allclose(edge[keep, 0:4], oe[keep, 0:4], rtol=CEILING, atol=CEILING * 1e-7 / 3e-5), (trial, edge[keep, 0:4], oe[keep, 0:4])
        assert np.allclose(edge[:, 7], oe[:, 7], rtol=CEILING), (trial, edge[:, 7], oe[:, 7])
    dev, ora = np.concatenate(dev_all), np.concatenate(ora_all)
    failures = []
    for key, cols, floor, host in (("sky/eval", slice(0, 3), 1e-7 / 3e-5, 3e-5), ("sky/pdf", slice(3, 4), 0.0, 3e-5), ("sky/sample", slice(4, 11), 1e-6 / 1e-4, 1e-4)):
        try:
            _check_values(key, dev[:, cols], ora[:, cols], floor, host)
        except AssertionError as e:
            failures.append(e)
    assert not failures, failures


def _light_cases():
    """The 3000 lights of test_lights_device_headers_match_oracle (same seed, same draws), then the edges."""
    rng = np.random.default_rng(9)
    lights, pos, xi = [], [], []
    for _ in range(3000):
        L = capi.MiGltfLight()
        L.type = int(rng.choice([capi.MI_LIGHT_DIRECTIONAL, capi.MI_LIGHT_POINT, capi.MI_LIGHT_SPOT]))
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        L.direction[:] = d.tolist()
        L.position[:] = rng.uniform(-3, 3, 3).tolist()
        L.color[:] = rng.uniform(0.1, 1, 3).tolist()
        L.intensity = rng.uniform(0.5, 50)
        L.radius = float(rng.choice([0.0, rng.uniform(0.05, 1.5)]))
        if L.type == capi.MI_LIGHT_DIRECTIONAL:
            L.angularSizeOrInvRange = float(rng.choice([0.0, rng.uniform(1e-4, 0.3)]))
        else:
            L.angularSizeOrInvRange = float(rng.choice([0.0, 1.0 / rng.uniform(2.0, 10.0)]))
        L.innerAngle = rng.uniform(0.0, 0.6)
        L.outerAngle = L.innerAngle + rng.uniform(0.0, 0.6)
        lights.append(L); pos.append(rng.uniform(-4, 4, 3)); xi.append(rng.random(2))
    n_random = len(lights)
    one_minus = float(np.nextafter(F32(1), F32(0)))
    for k in range(400):  # a point at the light, on a sphere light's surface, at `range` exactly, on a spot cone's inner and outer angle
        L = capi.MiGltfLight()
        L.type = int(capi.MI_LIGHT_SPOT if k % 5 >= 3 else capi.MI_LIGHT_POINT)
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        L.direction[:] = d.tolist()
        L.position[:] = rng.uniform(-3, 3, 3).tolist()
        L.color[:] = rng.uniform(0.1, 1, 3).tolist()
        L.intensity = rng.uniform(0.5, 50)
        L.radius, L.angularSizeOrInvRange = 0.0, 0.0
        L.innerAngle = rng.uniform(0.05, 0.6)
        L.outerAngle = L.innerAngle + rng.uniform(0.05, 0.6)
        lp = np.array(L.position[:], np.float64)
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        if k % 5 == 0:
            p = lp
            L.radius = float(rng.choice([0.0, 0.5]))
        elif k % 5 == 1:
            L.radius = rng.uniform(0.05, 1.5)
            p = lp + u * float(F32(L.radius))
        elif k % 5 == 2:
            rg = rng.uniform(2.0, 10.0)
            L.angularSizeOrInvRange = 1.0 / rg
            p = lp + u * rg
        else:
            ang = L.innerAngle if k % 5 == 3 else L.outerAngle
            t = np.cross(d, u); t /= np.linalg.norm(t)
            p = lp + (d * np.cos(ang) + t * np.sin(ang)) * rng.uniform(0.5, 5.0)
        lights.append(L); pos.append(p)
        xi.append([(0.0, one_minus, rng.random())[k % 3], (one_minus, 0.0, rng.random())[(k // 3) % 3]])
    arr = (capi.MiGltfLight * len(lights))(*lights)
    return arr, np.array(pos, F32), np.array(xi, F32), n_random


def test_lights_on_the_device_match_the_oracle():
    O = oracle_lib.lib()
    arr, pos, xi, n_random = _light_cases()
    dev = kat.light(arr, np.concatenate([pos, xi], 1))
    ora = np.zeros_like(dev)
    o8 = (F * 8)()
    for i in range(len(arr)):
        O.oracle_light_contribution(C.byref(arr[i]), (F * 3)(*pos[i]), (F * 2)(*xi[i]), o8)
        ora[i] = o8[:]
    # a delta light's pdf is the sentinel DIRAC = -1 (pt_math.h), every other pdf is a density
    assert np.isfinite(dev).all() and ((dev[:, 7] >= 0) | (dev[:, 7] == -1.0)).all() and (dev[:, 4:7] >= 0).all() and (dev[:, 3] >= 0).all()
    assert ((dev[:, 7] == -1.0) == (ora[:, 7] == -1.0)).all()
    # the edges against the oracle at the ceiling -- apart from the shading point ON a sphere light's surface (every fifth case from the second), where the
    # functions themselves are ill-conditioned in float32: cosMax = sqrt(1 - (radius / d)^2) at radius / d = 1 - O(ulp) is known to sqrt(ulp) = 3.5e-4 only,
    # and so is the cone direction (bound: 4 sqrt(ulp), absolute); the distance b - sqrt(b^2 - (d^2 - radius^2)) is a cancelled ~0 whose error grows with
    # 1 / b -- it is checked for its range alone (measured: device 1.4e-4, oracle 4.2e-4 for a true distance of 0).
    kind = np.full(len(arr), -1)
    kind[n_random:] = np.arange(len(arr) - n_random) % 5
    on_surface = kind == 1
    other = (kind >= 0) & ~on_surface
    assert np.allclose(dev[other], ora[other], rtol=CEILING, atol=CEILING * 1e-7 / 3e-5), (np.abs(dev[other] - ora[other]).max(0))
    assert np.abs(dev[on_surface, 0:3] - ora[on_surface, 0:3]).max() <= 4 * np.sqrt(EPS32)
    assert np.allclose(dev[on_surface, 4:8], ora[on_surface, 4:8], rtol=CEILING)
    radius = np.array([arr[i].radius for i in np.nonzero(on_surface)[0]])
    assert (dev[on_surface, 3] >= 0).all() and (dev[on_surface, 3] <= 2.0 * radius * (1 + 1e-5)).all()
    _check_values("lights", dev[:n_random], ora[:n_random], 1e-7 / 3e-5, 3e-5)
