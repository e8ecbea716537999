"""Restatements of the image-space denoisers of csrc/device/denoise.hip, shared by tests/test_gpu_denoise.py, tests/test_image_pass_reference.py and
tests/test_gpu_image_passes.py.

  * float64 (the reference every bound is against) and, with dtype=np.float32, the same expressions in the kernel's operation order (the
    conditioning of a case: how far float32 arithmetic alone moves the result).
  * per-pixel first-order error bounds of ONE iteration from the arithmetic of the kernel (see `Bounds` below).
  * an independent exact filter for inputs whose weights are all 0 or 1 (exact_filter): rational arithmetic, no code shared with the above.

Bounds.  u = 2^-24 is one float32 rounding.  The result of an iteration is out = sum(h_i q_i) / sum(h_i); a perturbation dh_i of the weights
moves it by sum(dh_i (q_i - out)) / sum(h_i) to first order, and the float32 evaluation of the sums and the quotient themselves costs at most
STRUCT_C roundings relative to max|input|:
      25 products q_i * h_i                       1   (each term carries one)
      25 running additions of the numerator      25
      25 running additions of sum(h)             25
      one division                                1
      h = kern * kern * w1 * w2 * w3 (3 products, kern * kern is exact) and up to 2 ulp (4 u) for each of three exp / pow factors
      landing next to 1                          12 (rounded up from 3 + 3 * 4 = 15 shared between numerator and denominator, of which
                                                     the common part cancels in the quotient)
                                                 --
      STRUCT_C                                   64      -> 64 * 2^-24 = 3.8e-6 of max|input| per iteration
Errors pass through later iterations convexly (every output is a weighted mean with non-negative weights), so they add and are not amplified.
A wrong tap weight (1/16 for 1/4) moves a pixel by about 1e-2 of the local contrast: more than three orders of magnitude above the bound.
dh_i per term (A = the exponent's argument, ULP2 = 4 u = two float32 ulp for a library or hardware transcendental):
      exp(-A):  dA from the roundings of the argument (counted at each term below) + A * u for the log2(e) product or the range reduction,
                dw = w * (dA + ULP2)
      nd ^ s:   dnd = 3 u * sum|n_q n_c| (3 products, 2 additions, absolute because the dot product cancels), dw = s nd^(s-1) dnd + w * ULP2
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
ULP2 = 4.0 * U
STRUCT_C = 64.0
LUMW = (0.2126, 0.7152, 0.0722)


def _work(dtype):
    """float64 restatements carry their sums, quotients and intermediate images in the widest float there is (80-bit on x86-64) and round once at
    the end: within 2 ulp of the exact rational filter over 8 iterations (tests/test_image_pass_reference.py).  float32 stays float32."""
    return np.longdouble if dtype is np.float64 else dtype


def _gather(H, W, oy, ox):
    ys, xs = np.arange(H) + oy, np.arange(W) + ox
    valid = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    return np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1), valid


def _lum(c):
    return LUMW[0] * c[..., 0] + LUMW[1] * c[..., 1] + LUMW[2] * c[..., 2]


def _pow_bound(nd, adot, s, w):
    """|d(nd^s)| for nd = max(0, dot) with |d dot| <= 3 u adot."""
    if s == 0:
        return ULP2 * w
    with np.errstate(all="ignore"):
        slope = s * np.where(nd > 0, nd ** (s - 1.0), 1.0 if s == 1 else 0.0)
    return slope * 3.0 * U * adot + ULP2 * w


def atrous_iteration(cur, albedo, normal, step, sigma_color, sigma_normal, sigma_albedo, dtype=np.float64, bound=False):
    """One k_atrous launch: (H, W, 4) -> (H, W, 4).  With bound=True also the per-pixel, per-channel error bound (H, W, 3) of a float32
    evaluation against this float64 one (module docstring)."""
    f = _work(dtype)
    H, W, _ = cur.shape
    kern = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f)
    cur, a, n = cur.astype(f), albedo.astype(f), normal.astype(f)
    solid = a[..., 3] > 0.5
    inv_c, inv_a = f(1.0) / max(f(sigma_color) * f(sigma_color), f(1e-8)), f(1.0) / max(f(sigma_albedo) * f(sigma_albedo), f(1e-8))
    acc, wsum, taps = np.zeros((H, W, 3), f), np.zeros((H, W), f), []
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx, valid = _gather(H, W, dy * step, dx * step)
                qc, qa, qn, qs = cur[qy][:, qx], a[qy][:, qx], n[qy][:, qx], solid[qy][:, qx]
                valid = valid & (qs == solid)
                arg_c = ((qc[..., :3] - cur[..., :3]) ** 2).sum(-1) * inv_c
                arg_a = ((qa[..., :3] - a[..., :3]) ** 2).sum(-1) * inv_a
                w_c, w_a = np.exp(-arg_c), np.exp(-arg_a)
                dot = (qn[..., :3] * n[..., :3]).sum(-1)
                nd = np.maximum(f(0.0), dot)
                w_n = np.where(solid, nd ** f(sigma_normal), f(1.0))
                k = kern[dy + 2] * kern[dx + 2]
                w = k * w_c * w_a * w_n * valid
                acc += qc[..., :3] * w[..., None]
                wsum += w
                if bound:
                    # argument of each exp: differences (u each, 3 u on the square), 2 additions, 1 / sigma^2 (2 u), the product, log2(e): 10 u A
                    e_exp = (10.0 * arg_c * U + ULP2) + (10.0 * arg_a * U + ULP2)
                    d_n = np.where(solid, _pow_bound(nd, np.abs(qn[..., :3] * n[..., :3]).sum(-1), sigma_normal, w_n), 0.0)
                    dw = k * valid * (w_c * w_a * w_n * (e_exp + 3.0 * U) + w_c * w_a * d_n + 1.2e-38)  # (+ a flushed denormal weight)
                    taps.append((dw, qc[..., :3]))
        out = cur.copy()
        ok = wsum > 0
        out[ok, :3] = acc[ok] / wsum[ok, None]
    if not bound:
        return out
    b = np.zeros((H, W, 3))
    for dw, qc in taps:
        b += (dw[..., None] * np.abs(qc - out[..., :3])).astype(np.float64)
    b = np.where(ok[..., None], b / np.where(ok, wsum, 1.0).astype(np.float64)[..., None], 0.0) + STRUCT_C * U * float(np.abs(cur[..., :3]).max())
    return out, b


def _atrous_numpy(img, albedo, normal, iterations, sigma_color, sigma_normal, sigma_albedo, dtype=np.float64):
    """Dammertz et al. 2010 edge-avoiding a-trous, B3-spline taps, weights = colour x albedo x normal^sigma, geometry is
    only filtered with geometry (albedo.w = first-hit fraction) -- the definition csrc/device/denoise.hip implements."""
    cur = img
    for it in range(iterations):
        cur = atrous_iteration(cur, albedo, normal, 1 << it, sigma_color, sigma_normal, sigma_albedo, dtype)
    return cur.astype(dtype)


def svgf_prepare(color, albedo, normal, frames, dtype=np.float64, bound=False):
    """k_svgf_prepare: ((illumination rgb, variance) (H, W, 4), demodulator (H, W, 3)); frames >= 4 takes the variance from the second moment
    in normal.w, fewer from the 7x7 neighbourhood.  With bound=True also |d variance| of a float32 evaluation."""
    f = _work(dtype)
    H, W, _ = color.shape
    c, a, n = color.astype(f), albedo.astype(f), normal.astype(f)
    solid = a[..., 3] > 0.5
    dem = np.where(solid[..., None], np.maximum(a[..., :3], f(0.02)), f(1.0))
    il = c[..., :3] / dem
    with np.errstate(all="ignore"):
        if frames >= 4:
            l, dl = _lum(c), _lum(dem)
            var = np.maximum(f(0.0), n[..., 3] - l * l) / f(frames) / (dl * dl)
            # m2 - l^2 cancels: l carries 3 u (so l^2 7 u), the difference one more of each operand; then two divisions and dl^2 (8 u)
            dvar = (np.where(n[..., 3] - l * l > -8.0 * U * l * l, (U * np.abs(n[..., 3]) + 8.0 * U * l * l) / frames / (dl * dl), 0.0) + 10.0 * U * var).astype(np.float64)
        else:
            li = _lum(il)
            s1, s2, sw = np.zeros((H, W), f), np.zeros((H, W), f), np.zeros((H, W), f)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    qy, qx, valid = _gather(H, W, dy, dx)
                    valid = valid & (solid[qy][:, qx] == solid)
                    nd = np.maximum(f(0.0), (n[qy][:, qx][..., :3] * n[..., :3]).sum(-1))
                    w = np.where(solid, (nd > f(0.9)).astype(f), f(1.0)) * valid
                    lq = li[qy][:, qx]
                    s1 += w * lq
                    s2 += w * lq * lq
                    sw += w
            m = np.where(sw > 0, s1 / np.maximum(sw, f(1e-30)), f(0.0))
            m2 = np.where(sw > 0, s2 / np.maximum(sw, f(1e-30)), f(0.0))
            var = np.where(sw > 0, np.maximum(f(0.0), m2 - m * m), f(0.0))
            # E[l^2] - E[l]^2 cancels: up to 49 running additions, l (4 u with the demodulation), the squares, the division: 60 u of E[l^2]
            dvar = (60.0 * U * m2).astype(np.float64)
    cur = np.concatenate([il, var[..., None]], -1)
    return (cur, dem, dvar) if bound else (cur, dem)


def svgf_iteration(cur, albedo, normal, depth, step, sigma_l, sigma_n, sigma_z, dtype=np.float64, bound=False, dvar=None):
    """One k_svgf_atrous launch over (illumination, variance).  With bound=True also the per-pixel error bound (H, W, 3) of the illumination
    of a float32 evaluation against this float64 one; dvar = |d variance| of the input (svgf_prepare)."""
    f = _work(dtype)
    H, W, _ = cur.shape
    cur, a, n = cur.astype(f), albedo.astype(f), normal.astype(f)
    solid = a[..., 3] > 0.5
    zk = f(1.0) / np.maximum(f(1.0) - depth.astype(f), f(1e-7))
    zx = np.empty_like(zk)
    zx[:, :-1] = zk[:, 1:]
    zx[:, -1] = zk[:, -2] if W > 1 else zk[:, -1]
    zy = np.empty_like(zk)
    zy[:-1] = zk[1:]
    zy[-1] = zk[-2] if H > 1 else zk[-1]
    gz = np.maximum(np.abs(zx - zk), np.abs(zy - zk))
    kern = {0: f(3 / 8), 1: f(1 / 4), 2: f(1 / 16)}
    gauss = {0: f(0.5), 1: f(0.25)}
    gv, gw, gdv = np.zeros((H, W), f), np.zeros((H, W), f), np.zeros((H, W))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qy, qx, valid = _gather(H, W, dy, dx)
            w = gauss[abs(dx)] * gauss[abs(dy)] * valid
            gv += w * cur[qy][:, qx][..., 3]
            gw += w
            if bound and dvar is not None:
                gdv += w * dvar[qy][:, qx]
    with np.errstate(all="ignore"):
        gvar = np.maximum(gv / gw, f(0.0))
        sdev = np.sqrt(gvar)
        lc = _lum(cur)
        h0 = kern[0] * kern[0]
        acc = cur[..., :3] * h0
        accv = cur[..., 3] * h0 * h0
        sw = np.full((H, W), h0, f)
        den_l = f(sigma_l) * sdev + f(1e-6)
        if bound:
            # 9 products and additions of the prefilter, the division: 12 u of it, on top of what the variance carries in; through the root
            dg = gdv / gw + 12.0 * U * gvar
            dsdev = np.minimum(np.sqrt(dg), dg / np.maximum(2.0 * sdev, 1e-300))
            dden_l = sigma_l * dsdev + 3.0 * U * den_l
            dgz = 3.0 * U * (np.maximum(zx, zy) + zk) * 2.0  # (each key 2 u: 1 - z and the reciprocal; the difference one more)
        taps = []
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                qy, qx, valid = _gather(H, W, dy * step, dx * step)
                valid = valid & (solid[qy][:, qx] == solid)
                qc = cur[qy][:, qx]
                lq = _lum(qc)
                arg_l = np.abs(lq - lc) / den_l
                w_l = np.exp(-arg_l)
                qn = n[qy][:, qx]
                nd = np.maximum(f(0.0), (qn[..., :3] * n[..., :3]).sum(-1))
                dist = f(step) * np.sqrt(f(dx * dx + dy * dy))
                w_n = nd ** f(sigma_n)
                zq = zk[qy][:, qx]
                den_z = f(sigma_z) * gz * dist + f(1e-6) * zk
                arg_z = np.abs(zq - zk) / den_z
                w_z = np.exp(-arg_z)
                w = np.where(solid, w_l * w_n * w_z, w_l) * valid
                k = kern[abs(dx)] * kern[abs(dy)]
                h = k * w
                acc += qc[..., :3] * h[..., None]
                accv += qc[..., 3] * h * h
                sw += h
                if bound:
                    # |lq - lc|: each luminance 4 u (demodulation, 3 products, 2 additions), absolute because the difference cancels -- but
                    # exactly 0 where the two pixels are the same numbers (one function of equal inputs); likewise the depth keys below
                    same_l = (qc[..., :3] == cur[..., :3]).all(-1)
                    da_l = np.where(same_l, 0.0, 4.0 * U * (np.abs(lq) + np.abs(lc)) / den_l) + arg_l * (dden_l / den_l + 3.0 * U)
                    d_l = w_l * (da_l + ULP2)
                    same_z = depth[qy][:, qx] == depth
                    da_z = np.where(same_z, 0.0, 3.0 * U * (zq + zk) / den_z) + arg_z * ((sigma_z * dist * dgz + 4.0 * U * den_z) / den_z + 3.0 * U)
                    d_z = w_z * (da_z + ULP2)
                    d_n = _pow_bound(nd, np.abs(qn[..., :3] * n[..., :3]).sum(-1), sigma_n, w_n)
                    d_geo = d_l * w_n * w_z + w_l * d_n * w_z + w_l * w_n * d_z + 3.0 * U * w_l * w_n * w_z
                    dh = k * valid * (np.where(solid, d_geo, d_l) + 1.2e-38)
                    taps.append((dh, qc[..., :3]))
        out = np.concatenate([acc / sw[..., None], (accv / (sw * sw))[..., None]], -1)
    if not bound:
        return out
    b = np.zeros((H, W, 3))
    for dh, qc in taps:
        b += (dh[..., None] * np.abs(qc - out[..., :3])).astype(np.float64)
    return out, b / sw.astype(np.float64)[..., None] + STRUCT_C * U * float(np.abs(cur[..., :3]).max())


def svgf_finish(cur, dem, color):
    out = np.empty(color.shape, cur.dtype)
    out[..., :3] = cur[..., :3] * dem
    out[..., 3] = color[..., 3]
    return out


def svgf_single(color, albedo, normal, depth, frames, sigma_l, sigma_n, sigma_z):
    """Prepare, ONE a-trous iteration and finish in float64: (output (H, W, 4), error bound of a float32 evaluation (H, W, 3),
    the intermediate (illumination, variance) (H, W, 4) after the iteration)."""
    cur, dem, dvar = svgf_prepare(color, albedo, normal, frames, bound=True)
    nxt, b = svgf_iteration(cur, albedo, normal, depth, 1, sigma_l, sigma_n, sigma_z, bound=True, dvar=dvar)
    scale = np.abs(color[..., :3].astype(np.float64)).max()
    out = svgf_finish(nxt, dem, color.astype(np.float64)).astype(np.float64)
    return out, b * dem.astype(np.float64) + 2.0 * U * scale, nxt.astype(np.float64)  # (+ demodulation and re-modulation)


def _svgf_numpy(color, albedo, normal, depth, frames, iterations, sigma_l, sigma_n, sigma_z, dtype=np.float64):
    """The definition csrc/device/denoise.hip implements (Schied et al. 2017 without reprojection), in float64."""
    cur, dem = svgf_prepare(color, albedo, normal, frames, dtype)
    for it in range(iterations):
        cur = svgf_iteration(cur, albedo, normal, depth, 1 << it, sigma_l, sigma_n, sigma_z, dtype)
    return svgf_finish(cur, dem, color.astype(dtype)).astype(dtype)


# ---- the independent computation: masked, renormalised 5x5 B3 spline at step 2^i in exact rational arithmetic ----------------------------
def exact_filter(values, kind, iterations, passes=None, centre_always=False):
    """values: H x W x 3 nested lists of int / Fraction; kind: H x W of bool (taps of the other kind are dropped); passes(y, x, qy, qx) -> bool:
    a further 0 / 1 factor on a tap (the axis-normal cases), asked for the centre too unless centre_always (the SVGF kernel adds the centre
    with weight 1 before its loop, k_atrous runs it through the weights like any tap).  A pixel with no tap left keeps its value."""
    H, W = len(values), len(values[0])
    b3 = (1, 4, 6, 4, 1)
    img = [[[Fraction(v) for v in px] for px in row] for row in values]
    for it in range(iterations):
        s = 1 << it
        nxt = []
        for y in range(H):
            row = []
            for x in range(W):
                num, den = [Fraction(0)] * 3, 0
                for j in range(5):
                    qy = y + (j - 2) * s
                    if not 0 <= qy < H:
                        continue
                    for i in range(5):
                        qx = x + (i - 2) * s
                        if not 0 <= qx < W or kind[qy][qx] != kind[y][x]:
                            continue
                        centre = i == 2 and j == 2
                        if passes is not None and not (centre and centre_always) and not passes(y, x, qy, qx):
                            continue
                        k = b3[i] * b3[j]
                        q = img[qy][qx]
                        num = [num[0] + k * q[0], num[1] + k * q[1], num[2] + k * q[2]]
                        den += k
                row.append([c / den for c in num] if den else img[y][x])
            nxt.append(row)
        img = nxt
    return img
