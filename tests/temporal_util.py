"""float64 numpy restatements for the motion-vector and temporal-reprojection tests, written from the reference's lines
(shaders/dlss_util.h:63-96 calculateMotionVector, shaders/gltf_pathtrace.slang:228-241 previous position of the first hit) and from
Schied et al. 2017 section 4.1 -- not from csrc/device/pt_temporal.h.  Shared by the CPU tier (tests/test_temporal_on_host.py, against
the header compiled for the host) and the GPU tier (tests/test_gpu_temporal.py, against the kernels)."""
import numpy as np

ID_INVALID = 0xFFFFFFFF
LUMW = np.array([0.2126, 0.7152, 0.0722])


def mat(a):
    """16 column-major floats -> 4x4 float64 matrix M with M @ column vector."""
    return np.asarray(a, np.float64).reshape(4, 4).T


def motion_numpy(first_hit, o2w, w2o, prev_o2w, view_proj, prev_mvp, width, height):
    """first_hit (N, 4) float32 (w = id bits); o2w / w2o / prev_o2w (K, 16) column-major.  Returns (N, 3) float64: motion x, y in pixels,
    previous NDC depth; and (N, 2) clip w under both cameras."""
    fh = np.asarray(first_hit, np.float32)
    ids = fh[:, 3].copy().view(np.uint32).astype(np.int64)
    p = fh[:, :3].astype(np.float64)
    vp, pm = mat(view_proj), mat(prev_mvp)
    out = np.zeros((len(fh), 3))
    clipw = np.ones((len(fh), 2))
    for i in range(len(fh)):
        if ids[i] == ID_INVALID:
            out[i] = (0.0, 0.0, 1.0)
            continue
        w = 1.0 if ids[i] else 0.0
        prev = p[i]
        if ids[i]:
            k = ids[i] - 1
            obj = mat(w2o[k]) @ np.append(p[i], 1.0)
            prev = (mat(prev_o2w[k]) @ np.append(obj[:3], 1.0))[:3]
        cur_clip, prev_clip = vp @ np.append(p[i], w), pm @ np.append(prev, w)
        cur_ndc, prev_ndc = cur_clip[:2] / cur_clip[3], prev_clip[:2] / prev_clip[3]
        out[i, :2] = (prev_ndc - cur_ndc) * 0.5 * np.array([width, height])
        out[i, 2] = prev_clip[2] / prev_clip[3] if ids[i] else 1.0
        clipw[i] = cur_clip[3], prev_clip[3]
    return out, clipw


def depth_key(ndc):
    return 1.0 / np.maximum(1.0 - ndc, 1e-7)


def demodulator(albedo):
    a = albedo.astype(np.float64)
    return np.where((a[..., 3] > 0.5)[..., None], np.maximum(a[..., :3], 0.02), 1.0)


def spatial_variance(il, albedo, normal):
    """7x7 variance of the demodulated luminance over neighbours of the same kind with a similar normal (paper section 4.2)."""
    H, W, _ = il.shape
    solid = albedo[..., 3] > 0.5
    n = normal.astype(np.float64)
    li = il @ LUMW
    s1, s2, sw = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            ys, xs = np.arange(H) + dy, np.arange(W) + dx
            valid = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
            qy, qx = np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)
            valid &= solid[qy][:, qx] == solid
            nd = np.maximum(0.0, (n[qy][:, qx][..., :3] * n[..., :3]).sum(-1))
            w = np.where(solid, (nd > 0.9).astype(np.float64), 1.0) * valid
            lq = li[qy][:, qx]
            s1 += w * lq
            s2 += w * lq * lq
            sw += w
    m = np.where(sw > 0, s1 / np.maximum(sw, 1e-30), 0.0)
    return np.where(sw > 0, np.maximum(0.0, s2 / np.maximum(sw, 1e-30) - m * m), 0.0)


def reproject_numpy(color, albedo, normal, depth, motion, hist, params, tainted=None):
    """One temporal stage.  hist: None (empty) or dict(illum (H,W,3), h (H,W), m1, m2, depth, id (uint32), normal (H,W,3)) in float64.
    params: dict(alpha, momentsAlpha, maxHistory, normalCos, depthTolerance).
    tainted: (H,W) bool, history pixels a float32 evaluation may have decided differently (None = none).
    Returns (new hist, illum+variance (H,W,4), valid taps (H,W) with 0 = reset, margin (H,W): the smallest relative distance of a tap
    decision of the pixel from its threshold, reads_tainted (H,W): a candidate tap of the pixel is a tainted history pixel)."""
    H, W, _ = color.shape
    c, n = color.astype(np.float64), normal.astype(np.float64)[..., :3]
    mv = motion.astype(np.float64)
    ids = np.ascontiguousarray(motion[..., 3]).view(np.uint32)
    il = c[..., :3] / demodulator(albedo)
    l1 = il @ LUMW
    l2 = l1 * l1
    acc = {k: np.zeros((H, W) + s) for k, s in (("illum", (3,)), ("h", ()), ("m1", ()), ("m2", ()))}
    wsum, taps, margin = np.zeros((H, W)), np.zeros((H, W), np.int64), np.full((H, W), np.inf)
    reads_tainted = np.zeros((H, W), bool)
    if hist is not None:
        ys, xs = np.mgrid[0:H, 0:W]
        # (pixel centre + motion) - 0.5: history texel coordinates; the sum is the one float32 operation restated as such, because it decides
        # WHICH texels are tapped (a float64 sum next to an integer could floor the other way)
        m32 = np.asarray(motion, np.float32)
        fx = (xs.astype(np.float32) + m32[..., 0]).astype(np.float64)
        fy = (ys.astype(np.float32) + m32[..., 1]).astype(np.float64)
        bx, by = np.floor(fx), np.floor(fy)
        tx, ty = fx - bx, fy - by
        kp = depth_key(mv[..., 2])
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = (bx + i).astype(np.int64), (by + j).astype(np.int64)
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                same = hist["id"][cy, cx] == ids
                dz = np.abs(depth_key(hist["depth"][cy, cx]) - kp)
                zok = dz <= params["depthTolerance"] * kp
                nd = (hist["normal"][cy, cx] * n).sum(-1)
                nok = (nd >= params["normalCos"]) | (ids == 0)
                valid = inside & same & zok & nok & (ids != ID_INVALID)
                # how close the float decisions were (id and inside are exact)
                cand = inside & same & (ids != ID_INVALID)
                mz = np.abs(dz / np.maximum(params["depthTolerance"] * kp, 1e-300) - 1.0)
                mn = np.where(ids == 0, np.inf, np.abs(nd - params["normalCos"]) / max(abs(params["normalCos"]), 1e-300))
                margin = np.where(cand, np.minimum(margin, np.minimum(mz, np.where(zok, mn, np.inf))), margin)
                if tainted is not None:
                    reads_tainted |= cand & tainted[cy, cx]
                w = (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty) * valid
                acc["illum"] += w[..., None] * hist["illum"][cy, cx]
                acc["h"] += w * hist["h"][cy, cx]
                acc["m1"] += w * hist["m1"][cy, cx]
                acc["m2"] += w * hist["m2"][cy, cx]
                wsum += w
                taps += valid
    keep = (taps > 0) & (wsum > 0)
    taps = np.where(keep, taps, 0)
    ws = np.where(keep, wsum, 1.0)
    h = np.where(keep, np.minimum(acc["h"] / ws + 1.0, params["maxHistory"]), 1.0)
    a = np.where(keep, np.maximum(params["alpha"], 1.0 / h), 1.0)
    am = np.where(keep, np.maximum(params["momentsAlpha"], 1.0 / h), 1.0)
    new = {
        "illum": acc["illum"] / ws[..., None] * (1.0 - a)[..., None] + il * a[..., None],
        "h": h,
        "m1": acc["m1"] / ws * (1.0 - am) + l1 * am,
        "m2": acc["m2"] / ws * (1.0 - am) + l2 * am,
        "depth": depth.astype(np.float64),
        "id": ids.copy(),
        "normal": n.copy(),
    }
    var_t = np.maximum(0.0, new["m2"] - new["m1"] ** 2)
    var = np.where(h >= 4.0, var_t, spatial_variance(il, albedo, normal))
    return new, np.concatenate([new["illum"], var[..., None]], -1), taps, margin, reads_tainted


def svgf_filter_numpy(cur, color, albedo, normal, depth, iterations, sigma_l, sigma_n, sigma_z):
    """The a-trous iterations and the re-modulation of Schied et al. 2017 (eq. 2-5) over a prepared (illumination, variance) image."""
    H, W, _ = cur.shape
    a, n = albedo.astype(np.float64), normal.astype(np.float64)
    solid = a[..., 3] > 0.5
    zk = depth_key(depth.astype(np.float64))
    zx, zy = np.empty_like(zk), np.empty_like(zk)
    zx[:, :-1], zx[:, -1] = zk[:, 1:], zk[:, -2]
    zy[:-1], zy[-1] = zk[1:], zk[-2]
    gz = np.maximum(np.abs(zx - zk), np.abs(zy - zk))
    kern, gauss = {0: 3 / 8, 1: 1 / 4, 2: 1 / 16}, {0: 0.5, 1: 0.25}

    def shifted(dy, dx):
        ys, xs = np.arange(H) + dy, np.arange(W) + dx
        valid = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
        return np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1), valid

    for it in range(iterations):
        step = 1 << it
        gv, gw = np.zeros((H, W)), np.zeros((H, W))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                qy, qx, valid = shifted(dy, dx)
                w = gauss[abs(dx)] * gauss[abs(dy)] * valid
                gv += w * cur[qy][:, qx][..., 3]
                gw += w
        sdev = np.sqrt(np.maximum(gv / gw, 0.0))
        lc = cur[..., :3] @ LUMW
        h0 = kern[0] * kern[0]
        acc, accv, sw = cur[..., :3] * h0, cur[..., 3] * h0 * h0, np.full((H, W), h0)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                qy, qx, valid = shifted(dy * step, dx * step)
                valid = valid & (solid[qy][:, qx] == solid)
                qc = cur[qy][:, qx]
                w = np.exp(-np.abs(qc[..., :3] @ LUMW - lc) / (sigma_l * sdev + 1e-6))
                nd = np.maximum(0.0, (n[qy][:, qx][..., :3] * n[..., :3]).sum(-1))
                dist = step * np.sqrt(dx * dx + dy * dy)
                wg = nd ** sigma_n * np.exp(-np.abs(zk[qy][:, qx] - zk) / (sigma_z * gz * dist + 1e-6 * zk))
                hw = kern[abs(dx)] * kern[abs(dy)] * np.where(solid, w * wg, w) * valid
                acc += qc[..., :3] * hw[..., None]
                accv += qc[..., 3] * hw * hw
                sw += hw
        cur = np.concatenate([acc / sw[..., None], (accv / (sw * sw))[..., None]], -1)
    out = np.empty((H, W, 4))
    out[..., :3] = cur[..., :3] * demodulator(albedo)
    out[..., 3] = color[..., 3]
    return out
