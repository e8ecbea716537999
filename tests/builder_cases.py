"""Geometry made to stress the decisions of the acceleration-structure builder (csrc/device/bvh_build.hip, bvh8.hip, bvh_split.h,
bvh_reinsert.h), for tests/test_builder_cases_reference.py (CPU) and tests/test_gpu_builder_matrix.py (GPU): per case a .glb written with
scenegen.GlbBuilder, its own recipe of 1024 rays, the render nodes the float64 reference is computed on, and -- MEASURED -- the float32 error of
the ray / triangle test on the case's own unambiguous pairs (query_util.measure_float32_error), which the GPU tolerance is 8 x.  Also float32
restatements of the two builder stages whose outcome a case relies on: k_morton's quantisation (the keys) and the PLOC clustering rounds
(k_ploc_nn + k_ploc_flags: the depth of the BVH2).  Pure numpy, no GPU."""
import os

import numpy as np

import query_util as qu

F32 = np.float32
NUM_RAYS = 1024
COUNTS = (2, 3, 8, 9, 17, 33, 255, 256, 257, 272, 273, 513)  # (256 = one block of k_ploc_nn, 256 +- PLOC_RADIUS = its LDS halo)
CHAINS = {"chain130": (130, 1.05), "chain600": (600, 1.03)}  # shells, ratio
NAMES = tuple("counts_%d" % n for n in COUNTS) + ("one_cell", "copies", "flat_x", "flat_y", "flat_z", "line", "offset", "scales", "needles") + tuple(CHAINS)

# (|t32 - t64| / max(1, t64), max(|u32 - u64|, |v32 - v64|)) of the float32 ray / triangle test against float64 on the unambiguous pairs of each
# case's own rays: MEASURED on the CPU by query_util.measure_float32_error (tests/test_builder_cases_reference.py re-measures and fails above these);
# the GPU tolerance is 8 x, the margin query_util.TOLERANCE takes for the one rounding the device adds when it forms the world-space edges.
MEASURED = {
    "counts_2": (8.7510e-06, 1.1523e-04),  # 2 triangles, 726 of 1024 rays hit, 0.0000 % ambiguous
    "counts_3": (3.3256e-06, 7.1463e-05),  # 3 triangles, 755 of 1024 rays hit, 0.0000 % ambiguous
    "counts_8": (3.8146e-06, 5.4332e-05),  # 8 triangles, 735 of 1024 rays hit, 0.0000 % ambiguous
    "counts_9": (6.1938e-06, 7.5643e-05),  # 9 triangles, 718 of 1024 rays hit, 0.0000 % ambiguous
    "counts_17": (1.3208e-03, 4.0760e-03),  # 17 triangles, 724 of 1024 rays hit, 0.0000 % ambiguous
    "counts_33": (3.7125e-05, 9.0267e-04),  # 33 triangles, 731 of 1024 rays hit, 0.0977 % ambiguous
    "counts_255": (4.3266e-05, 1.1079e-04),  # 255 triangles, 844 of 1024 rays hit, 0.0977 % ambiguous
    "counts_256": (6.9500e-06, 7.0962e-05),  # 256 triangles, 843 of 1024 rays hit, 0.0977 % ambiguous
    "counts_257": (1.5003e-05, 2.3954e-04),  # 257 triangles, 873 of 1024 rays hit, 0.0000 % ambiguous
    "counts_272": (3.1610e-05, 6.7540e-04),  # 272 triangles, 848 of 1024 rays hit, 0.1953 % ambiguous
    "counts_273": (3.0077e-05, 3.7178e-04),  # 273 triangles, 840 of 1024 rays hit, 0.0000 % ambiguous
    "counts_513": (4.9982e-06, 8.9411e-05),  # 513 triangles, 923 of 1024 rays hit, 0.0000 % ambiguous
    "one_cell": (2.7946e-06, 1.7601e-04),  # 502 triangles, 954 of 1024 rays hit, 0.4883 % ambiguous
    "copies": (1.1349e-07, 1.1993e-06),  # 1280 triangles, 885 of 1024 rays hit, 0.0000 % ambiguous
    "flat_x": (2.2244e-07, 4.2043e-06),  # 512 triangles, 972 of 1024 rays hit, 0.0000 % ambiguous
    "flat_y": (2.6510e-07, 6.0534e-06),  # 512 triangles, 966 of 1024 rays hit, 0.0000 % ambiguous
    "flat_z": (2.5441e-07, 4.0952e-06),  # 512 triangles, 962 of 1024 rays hit, 0.0000 % ambiguous
    "line": (3.2033e-06, 2.5096e-03),  # 300 triangles, 732 of 1024 rays hit, 0.1953 % ambiguous
    "offset": (6.3709e-06, 5.4488e-05),  # 576 triangles, 965 of 1024 rays hit, 0.0977 % ambiguous
    "scales": (2.9409e-07, 1.3389e-07),  # 104 triangles, 985 of 1024 rays hit, 0.0000 % ambiguous
    "needles": (1.6907e-04, 1.0681e-02),  # 564 triangles, 946 of 1024 rays hit, 0.2930 % ambiguous
    "chain130": (3.6527e-06, 1.3786e-07),  # 130 triangles, 1024 of 1024 rays hit, 0.0000 % ambiguous
    "chain600": (9.3020e-06, 1.1368e-07),  # 600 triangles, 1024 of 1024 rays hit, 0.0000 % ambiguous
}
TOLERANCE = {k: (8.0 * t, 8.0 * b) for k, (t, b) in MEASURED.items()}


# ---- float32 restatements of builder stages -----------------------------------------------------------------------------------------------------
def expand_bits21(v):
    """expandBits21 of bvh_build.hip: bit i of a 21-bit number to bit 3 i."""
    x = v.astype(np.uint64) & np.uint64(0x1fffff)
    for shift, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def boxes32(V32):
    """The float32 boxes of the world triangles, as k_tri_setup forms them."""
    return V32.min(1).astype(F32), V32.max(1).astype(F32)


def morton(V32):
    """k_morton in float32: (keys, the three 21-bit cells) of every triangle from the centres of its box and the bounds of those centres."""
    lo, hi = boxes32(V32)
    cen = F32(0.5) * (lo + hi)
    blo, bhi = cen.min(0), cen.max(0)
    ext = bhi - blo
    with np.errstate(all="ignore"):
        n = np.where(ext > 0, (cen - blo) / ext, F32(0)).astype(F32)
    q = np.minimum(np.maximum(n * F32(2097152.0), F32(0)), F32(2097151.0)).astype(np.uint32)
    keys = (expand_bits21(q[:, 0]) << np.uint64(2)) | (expand_bits21(q[:, 1]) << np.uint64(1)) | expand_bits21(q[:, 2])
    return keys, q


PLOC_RADIUS = 16


def ploc_depth(V32):
    """The height of the BVH2 the PLOC rounds of buildBvh make of these triangles (no pre-splitting, before reinsertion), and the number of rounds:
    leaves in stable key order, per round every cluster's nearest neighbour within PLOC_RADIUS positions by the float32 area of the union -- summed as
    k_ploc_nn sums it, ties to the smaller position -- and mutual pairs merged into the smaller position (k_ploc_flags, k_ploc_emit)."""
    keys, _ = morton(V32)
    order = np.argsort(keys, kind="stable")
    lo, hi = boxes32(V32)
    lo, hi = lo[order], hi[order]
    depth = np.zeros(len(lo), np.int64)
    rounds = 0
    while len(lo) > 1:
        m = len(lo)
        best = np.full(m, np.inf, F32)
        nn = np.full(m, -1)
        idx = np.arange(m)
        for d in range(-PLOC_RADIUS, PLOC_RADIUS + 1):  # ascending position: `a < best` keeps the smaller one on a tie
            g = idx + d
            ok = (d != 0) & (g >= 0) & (g < m)
            gc = np.clip(g, 0, m - 1)
            e = (np.maximum(hi, hi[gc]) - np.minimum(lo, lo[gc])).astype(F32)
            a = ((e[:, 0] * e[:, 1]).astype(F32) + (e[:, 1] * e[:, 2]).astype(F32)).astype(F32) + (e[:, 2] * e[:, 0]).astype(F32)
            take = ok & (a.astype(F32) < best)
            best[take], nn[take] = a.astype(F32)[take], g[take]
        mutual = (nn >= 0) & (nn[np.clip(nn, 0, m - 1)] == idx)
        first, second = mutual & (idx < nn), mutual & (idx > nn)
        assert first.any(), "a PLOC round made no progress"
        j = nn[first]
        lo[first], hi[first] = np.minimum(lo[first], lo[j]), np.maximum(hi[first], hi[j])
        depth[first] = 1 + np.maximum(depth[first], depth[j])
        lo, hi, depth = lo[~second], hi[~second], depth[~second]
        rounds += 1
    return int(depth[0]), rounds


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------
def _save(path, parts):
    """parts: [(positions (V, 3), triangles (T, 3) or None = every three vertices, [node keywords, ...])], one mesh each."""
    from vk_gltf_renderer_amd import scenegen
    b = scenegen.GlbBuilder()
    for pos, idx, nodes in parts:
        pos = np.asarray(pos, F32).reshape(-1, 3)
        idx = np.arange(len(pos), dtype=np.uint32).reshape(-1, 3) if idx is None else np.asarray(idx, np.uint32)
        mesh = b.mesh([b.primitive(pos, idx)])
        for kw in nodes:
            b.node(mesh=mesh, **kw)
    return b.save(path)


def _cloud(rng, n, lo, hi, size):
    """n triangles: centres uniform in [lo, hi]^3, vertices within `size` of them."""
    c = rng.uniform(lo, hi, size=(n, 1, 3))
    return (c + rng.uniform(-size, size, size=(n, 3, 3))).astype(F32)


def _sheet(rng, n, cell, jitter):
    """An (n x n)-quad sheet in the plane of the first two coordinates: (vertices (., 2), triangles)."""
    u, v = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy")
    p = np.stack([u.reshape(-1), v.reshape(-1)], 1).astype(np.float64) + rng.uniform(-jitter, jitter, size=((n + 1) ** 2, 2))
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    idx = np.stack([i, i + 1, i + n + 2, i, i + n + 2, i + n + 1], 1).reshape(-1, 3)
    return p * cell, idx


def _chain_sizes(name):
    shells, ratio = CHAINS[name]
    return np.array([float(F32(ratio ** k)) for k in range(shells)])


def make_scene(name, directory):
    """Writes the scene of case `name` into `directory`, returns its path."""
    path = os.path.join(str(directory), name + ".glb")
    rng = np.random.default_rng(1000 + NAMES.index(name))
    if name.startswith("counts_"):
        return _save(path, [(_cloud(rng, int(name[7:]), 0.1, 0.9, 0.08), None, [{}])])
    if name == "one_cell":
        # the two far triangles stretch the centroid bounds to [-2^20, 2^20]: a Morton cell is one unit wide and holds the whole cluster
        far = np.array([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]], np.float64)
        tris = np.concatenate([_cloud(rng, 500, 0.03, 0.22, 0.025), (far + 2.0 ** 20)[None], (far - 2.0 ** 20)[None]])
        return _save(path, [(tris, None, [{}])])
    if name == "copies":
        from vk_gltf_renderer_amd import scenegen
        pos, _, _, idx = scenegen.grid(4, 4, (1.0, 1.0), "y")
        return _save(path, [(pos, idx, [{"translation": [0.5, 0.25, -0.125]}] * 40)])
    if name in ("flat_x", "flat_y", "flat_z"):
        axis = "xyz".index(name[5])
        p2, idx = _sheet(rng, 16, 0.25, 0.3)
        pos = np.full((len(p2), 3), 3.3)
        pos[:, [a for a in range(3) if a != axis]] = p2
        return _save(path, [(pos, idx, [{}])])
    if name == "line":
        # box centres (x_i, 1.5, -2.25): every number a multiple of 2^-10, so that the float32 boxes and their centres are exact
        q = 2.0 ** -10
        cx = rng.permutation(4096)[:300] * (8 * q)
        c = np.stack([cx, np.full(300, 1.5), np.full(300, -2.25)], 1)
        h = rng.integers(8, 64, size=(300, 3)) * q
        h[:, 0] = rng.integers(8, 20, size=300) * q  # (short along the line: few overlap, few near-ties in t for the reference to set aside)
        w = rng.integers(-7, 8, size=(300, 3)) * q
        sx, sy, sz = np.eye(3)
        tris = np.stack([c - h * (sx + sy) + w * sz, c + h * (sx - sz) + w * sy, c + h * (sy + sz) + w * sx], 1)
        return _save(path, [(tris, None, [{}])])
    if name == "offset":
        q = 2.0 ** -6
        parts_p, parts_i = [], []
        for layer in range(2):
            p2, idx = _sheet(rng, 12, 0.5, 0.3)
            p = np.concatenate([p2, np.full((len(p2), 1), float(layer)) + rng.uniform(-0.2, 0.2, size=(len(p2), 1))], 1)
            parts_i.append(idx + layer * len(p2))
            parts_p.append(np.round(p / q) * q)
        return _save(path, [(np.concatenate(parts_p), np.concatenate(parts_i), [{"translation": [65536.0, 65536.0, 65536.0]}])])
    if name == "scales":
        tris = []
        for k in range(-3, 4):
            for half in (1.0, np.sqrt(10.0)):
                if k == 3 and half > 1.0:
                    break
                r = half * 10.0 ** k
                for sx in (-1, 1):
                    for sy in (-1, 1):
                        for sz in (-1, 1):
                            tris.append([[sx * r, 0, 0], [0, sy * r, 0], [0, 0, sz * r]])
        return _save(path, [(np.array(tris), None, [{}])])
    if name == "needles":
        d = rng.uniform(0.3, 1.0, size=(64, 3)) * rng.choice([-1.0, 1.0], size=(64, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        p = rng.uniform(-2.0, 2.0, size=(64, 3))
        side = np.cross(d, rng.normal(size=(64, 3)))
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        a, b = p - 500.0 * d, p + 500.0 * d
        # (the first vertex at the wide end: one edge of the ray / triangle test is then the short one, and its float32 determinant no difference of
        #  products a million times its size)
        needles = np.stack([b, b + 1e-2 * side, a], 1)
        return _save(path, [(np.concatenate([needles.astype(F32), _cloud(rng, 500, -2.0, 2.0, 0.5)]), None, [{}])])
    # the nested corner triangles (s, 0, 0), (0, s, 0), (0, 0, s): boxes [0, s]^3, one render node per shell
    s = _chain_sizes(name)
    return _save(path, [(np.eye(3), None, [{"scale": [v, v, v]} for v in s])])


def reference_nodes(name):
    """The render nodes the float64 reference of the case is computed on (None: all).  `copies` stacks 40 exact copies: the reference is the first
    alone, and the exact-tie rule of the query (pt_query.h: ties to the smaller (renderNode, triangle)) makes every hit report that one."""
    return {0} if name == "copies" else None


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------------
def _on_triangles(V, share):
    """make_rays' `aim`: `share` of the rays aim at a point well inside a random triangle of V, the others where the recipe aimed them."""
    def aim(rng, target):
        n = len(target)
        k = rng.integers(0, len(V), size=n)
        w = rng.dirichlet(np.ones(3), size=n) * 0.7 + 0.1  # (every barycentric coordinate >= 0.1)
        p = (V[k] * w[:, :, None]).sum(1)
        return np.where((rng.uniform(size=n) < share)[:, None], p, target)
    return aim


def _pack(o, d):
    rays = np.zeros(len(o), qu.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tMin"], rays["tMax"] = o, d / np.linalg.norm(d, axis=1, keepdims=True), 0.0, np.inf
    return rays


def make_rays(name, st):
    """The 1024 rays of case `name` over its triangles `st` (query_util.SceneTris of reference_nodes)."""
    seed = 2000 + NAMES.index(name)
    if name.startswith("counts_"):
        return qu.make_rays(st, NUM_RAYS, seed, aim=_on_triangles(st.V, 0.7))
    if name in ("one_cell", "needles"):  # at the cluster, not at the scene's bounds
        near = st.V[np.abs(st.V).max((1, 2)) < 4.0] if name == "one_cell" else st.V[64:]
        V = near
        if name == "needles":  # ... and one ray in nine at a point of a needle where it crosses the cluster (s: along it, l: across)
            b, c, a = (st.V[:64, i] for i in range(3))
            r = np.random.default_rng(seed + 500)
            s, l = r.uniform(0.4985, 0.5015, size=(64, 1)), r.uniform(0.2, 0.8, size=(64, 1))
            mid = a + s * (b - a) + s * l * (c - b)
            V = np.concatenate([near, np.repeat(mid[:, None], 3, 1)])
        return qu.make_rays(st, NUM_RAYS, seed, bounds=(near.min((0, 1)), near.max((0, 1))), aim=_on_triangles(V, 0.7))
    if name in ("copies", "offset", "flat_x", "flat_y", "flat_z", "line"):
        pad = np.where(st.hi - st.lo < 0.5, 1.0, 0.0)  # (a flat or thin scene: origins off its plane or line)
        rays = qu.make_rays(st, NUM_RAYS, seed, bounds=(st.lo - pad, st.hi + pad), aim=_on_triangles(st.V, 0.7))
        if name.startswith("flat_"):  # half of them perpendicular to the sheet instead
            axis = "xyz".index(name[5])
            r = np.random.default_rng(seed + 500)
            p = _on_triangles(st.V, 1.0)(r, np.zeros((NUM_RAYS // 2, 3)))
            d = np.zeros_like(p)
            d[:, axis] = r.choice([-1.0, 1.0], size=len(p))
            rays[::2] = _pack(p - d * r.uniform(0.5, 3.0, size=(len(p), 1)), d)
        return rays
    rng = np.random.default_rng(seed)
    if name == "scales":
        # from between two shells (L1 radius rho between theirs; k = 13: beyond the last), outward or inward
        radii = np.sort(np.abs(st.V).max((1, 2)))[::8]
        k = rng.integers(0, len(radii) + 1, size=NUM_RAYS)
        inner = np.where(k > 0, radii[np.maximum(k - 1, 0)], 0.0)
        outer = np.where(k < len(radii), radii[np.minimum(k, len(radii) - 1)], 3.0 * radii[-1])
        rho = inner + (outer - inner) * rng.uniform(0.3, 0.7, size=NUM_RAYS)
        w = (rng.dirichlet(np.ones(3), size=NUM_RAYS) * 0.7 + 0.1) * rng.choice([-1.0, 1.0], size=(NUM_RAYS, 3))
        o = w * rho[:, None]
        aim_in = (rng.dirichlet(np.ones(3), size=NUM_RAYS) * 0.7 + 0.1) * rng.choice([-1.0, 1.0], size=(NUM_RAYS, 3)) * (0.4 * inner)[:, None]
        outward = np.sign(w) * rng.uniform(0.2, 1.0, size=(NUM_RAYS, 3))
        go_in = (rng.uniform(size=NUM_RAYS) < 0.5) & (k > 0)
        return _pack(o, np.where(go_in[:, None], aim_in - o, outward))
    # chains: half from between shells k - 1 and k, outward (the hit is shell k); half from beyond the last shell towards the common corner
    s = _chain_sizes(name)
    half = NUM_RAYS // 2
    k = rng.integers(0, len(s), size=half)
    below = np.where(k > 0, s[np.maximum(k - 1, 0)], 0.0)
    rho = below + (s[k] - below) * rng.uniform(0.2, 0.8, size=half)
    o1 = (rng.dirichlet(np.ones(3), size=half) * 0.7 + 0.1) * rho[:, None]
    d1 = rng.uniform(0.2, 1.0, size=(half, 3))
    o2 = (rng.dirichlet(np.ones(3), size=half) * 0.7 + 0.1) * (s[-1] * rng.uniform(1.5, 3.0, size=half))[:, None]
    t2 = (rng.dirichlet(np.ones(3), size=half) * 0.7 + 0.1) * (0.2 * s[0])
    return np.concatenate([_pack(o1, d1), _pack(o2, t2 - o2)])
