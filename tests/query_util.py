"""Shared helpers of the ray-query tests (tests/test_gpu_query.py, tests/test_query_reference.py): the world-space triangles of a scene
description in float64, the ray recipe, a float64 brute-force Moeller-Trumbore closest hit with the ambiguity classes the GPU test allows
for, and the triangle / shade records of the device as arrays (for tests/host_shim/query_on_host.cpp).  No GPU needed."""
import numpy as np

F32 = np.float32
DELTA = 1e-4  # barycentric units: how close to an edge, or (x max(1, t)) to another surface, a float64 hit may lie before float32 may disagree

RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("tMin", "<f4"), ("direction", "<f4", (3,)), ("tMax", "<f4")])
TRI_DTYPE = np.dtype([("v0", "<f4", (3,)), ("rnode", "<u4"), ("e1", "<f4", (3,)), ("prim", "<u4"), ("e2", "<f4", (3,)), ("flags", "<u4")])
SHADE_DTYPE = np.dtype([("v0", "<u4"), ("v1", "<u4"), ("v2", "<u4"), ("rnode", "<u4"), ("renderPrimID", "<i4"), ("materialID", "<i4"), ("prim", "<u4"),
                        ("attrs", "<u4")])
INST_FLIP_FACING = 4

# The scenes of the reference comparison and, per scene, the largest difference between the float32 ray / triangle test (oracle_intersect_tri: the
# device's test bit for bit, on world vertices rounded as the build rounds them) and the float64 formula on the unambiguous (ray, nearest
# triangle) pairs of make_rays(seed 7, 2048 rays): (|t32 - t64| / max(1, t64), max(|u32 - u64|, |v32 - v64|)).  MEASURED on the CPU by
# measure_float32_error below (tests/test_query_reference.py re-measures and compares); the tolerance of the GPU test is 8 x these -- the margin
# covers the one rounding the device adds when it forms the world-space edges.  (The sliver atrium's thin triangles amplify the rounding of their
# world vertices, 2e-6 at 20 units from the origin, into barycentric errors above DELTA: the largest figures by far.)
# Ambiguous shares of the same rays under the float64 reference alone: animated 0.05 %, variants 0.00 %, mixed 0.00 %, sliver atrium (detail
# 0.25) 0.20 %; the cap the tests assert is 1 %.
MEASURED = {
    "animated": (3.417e-07, 1.059e-05),
    "variants": (1.025e-06, 5.913e-05),
    "mixed_alpha_glass": (8.564e-07, 3.020e-05),
    "atrium_sliver": (7.277e-05, 1.905e-04),
}
TOLERANCE = {k: (8.0 * t, 8.0 * b) for k, (t, b) in MEASURED.items()}
MAX_AMBIGUOUS_SHARE = 0.01


def make_scene(name, directory):
    """Writes the scene `name` of MEASURED into `directory`, returns its path."""
    import os
    from vk_gltf_renderer_amd import scenegen
    path = os.path.join(str(directory), name + ".glb")
    if name == "animated":
        return scenegen.scene_animated(path)
    if name == "variants":
        return scenegen.scene_variants(path)
    if name == "mixed_alpha_glass":
        return scenegen.scene_mixed_alpha_glass(path)
    assert name == "atrium_sliver"
    return scenegen.scene_atrium_class(path, detail=0.25, tex_size=64, sliver=True)


def measure_float32_error(st, rays, ref):
    """MEASURED's pair for one scene: oracle_intersect_tri against the float64 reference on the unambiguous hits."""
    import ctypes as C
    import oracle_lib
    O = oracle_lib.lib()
    P = C.POINTER(C.c_float)
    tri9 = np.ascontiguousarray(np.concatenate([st.V32[:, 0], st.V32[:, 1] - st.V32[:, 0], st.V32[:, 2] - st.V32[:, 0]], 1), F32)
    o5 = (C.c_float * 5)()
    err_t = err_b = 0.0
    for i in np.nonzero(~ref.ambiguous & ref.hit)[0]:
        o, d = np.ascontiguousarray(rays["origin"][i]), np.ascontiguousarray(rays["direction"][i])
        O.oracle_intersect_tri(tri9[ref.tri[i]].ctypes.data_as(P), o.ctypes.data_as(P), d.ctypes.data_as(P), o5)
        assert o5[0] == 1.0, ("float32 misses an unambiguous float64 hit", int(i))
        err_t = max(err_t, abs(o5[1] - ref.t[i]) / max(1.0, ref.t[i]))
        err_b = max(err_b, abs(o5[2] - ref.u[i]), abs(o5[3] - ref.v[i]))
    return err_t, err_b


class SceneTris:
    """Every triangle of every visible render node of a scene description, in world space."""

    def __init__(self, scene, nodes=None):
        """nodes: the render nodes to take (default: every visible one)."""
        d = scene.desc.contents
        V, V32, node, prim, tri, mat, flip = [], [], [], [], [], [], []
        for n in range(d.numRenderNodes):
            rn = d.renderNodes[n]
            if nodes is not None and n not in nodes:
                continue
            if d.renderNodeVisible and not d.renderNodeVisible[n]:
                continue
            if rn.renderPrimID < 0 or rn.renderPrimID >= d.numRenderPrimitives:
                continue
            rp = d.renderPrimitives[rn.renderPrimID]
            if rp.triangleCount == 0:
                continue
            idx = np.ctypeslib.as_array(rp.indices, shape=(rp.triangleCount, 3)).astype(np.int64)
            pos = np.ctypeslib.as_array(rp.positions, shape=(rp.vertexCount, 3))
            M32 = np.array(rn.objectToWorld[:], F32).reshape(4, 4).T  # (column-major in memory)
            M = M32.astype(np.float64)
            w = pos.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
            V.append(w[idx])
            # the device's vertices: mulPoint in float32 (pt_math.h: a chain of three fmas from the translation)
            w32 = np.empty_like(pos)
            for r in range(3):
                acc = np.full(len(pos), M32[r, 3], F32)
                for c in range(3):
                    acc = (acc.astype(np.float64) + M[r, c] * pos[:, c].astype(np.float64)).astype(F32)  # (a float64 product of floats is exact: one rounding)
                w32[:, r] = acc
            V32.append(w32[idx])
            k = int(rp.triangleCount)
            node.append(np.full(k, n)); prim.append(np.full(k, rn.renderPrimID)); tri.append(np.arange(k)); mat.append(np.full(k, max(0, rn.materialID)))
            flip.append(np.full(k, np.linalg.det(M[:3, :3]) < 0))
        cat = lambda parts, dt, shape: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
        self.V = cat(V, np.float64, (0, 3, 3))
        self.V32 = cat(V32, F32, (0, 3, 3))
        self.node, self.prim, self.tri, self.mat = (cat(x, np.int64, (0,)) for x in (node, prim, tri, mat))
        self.flip = cat(flip, bool, (0,))
        self.v0, self.e1, self.e2 = self.V[:, 0], self.V[:, 1] - self.V[:, 0], self.V[:, 2] - self.V[:, 0]
        self.lo, self.hi = (self.V.min((0, 1)), self.V.max((0, 1))) if len(self.V) else (np.zeros(3), np.zeros(3))
        self.radius = float(0.5 * np.linalg.norm(self.hi - self.lo))
        self.size = 4.0 * self.radius  # no ray of the recipe below travels further than 2.5 radii to a hit

    def __len__(self):
        return len(self.V)

    def device_records(self):
        """(DevTri, DevShadeTri) arrays, one slot per triangle: world vertices and edges rounded as the build rounds them."""
        t, s = np.zeros(len(self), TRI_DTYPE), np.zeros(len(self), SHADE_DTYPE)
        t["v0"], t["e1"], t["e2"] = self.V32[:, 0], self.V32[:, 1] - self.V32[:, 0], self.V32[:, 2] - self.V32[:, 0]
        t["rnode"], t["prim"], t["flags"] = self.node, self.tri, np.where(self.flip, INST_FLIP_FACING, 0)
        s["rnode"], s["renderPrimID"], s["materialID"], s["prim"] = self.node, self.prim, self.mat, self.tri
        return t, s


def make_rays(st, n=2048, seed=7, bounds=None, aim=None):
    """Half of the origins on a sphere of 1.5 x the bounds' radius around their centre, half inside the bounds; every ray aims at a uniform
    point of the bounds.  Unit directions, tMin 0, no far bound.
    bounds: (lo, hi) to use instead of the scene's; aim(rng, uniform targets) -> the (n, 3) points the rays aim at instead."""
    rng = np.random.default_rng(seed)
    lo, hi = (st.lo, st.hi) if bounds is None else (np.asarray(bounds[0], np.float64), np.asarray(bounds[1], np.float64))
    radius = st.radius if bounds is None else float(0.5 * np.linalg.norm(hi - lo))
    c = 0.5 * (lo + hi)
    on = rng.normal(size=(n // 2, 3))
    on = c + 1.5 * radius * on / np.linalg.norm(on, axis=1, keepdims=True)
    inside = rng.uniform(lo, hi, size=(n - n // 2, 3))
    o = np.concatenate([on, inside])
    target = rng.uniform(lo, hi, size=(n, 3))
    if aim is not None:
        target = aim(rng, target)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tMin"], rays["tMax"] = o, d, 0.0, np.inf
    return rays


def as_rows(rays):
    """The (n, 8) float32 view PathTracer.query_rays takes."""
    return rays.view(F32).reshape(-1, 8)


class Pairs:
    """float64 Moeller-Trumbore of every ray against every triangle its line comes near: the sparse list of (ray, triangle, t, u, v, det) with
    the hit inside the DELTA-enlarged triangle, whatever its t.  Computed once per (scene, rays); Reference applies the ray intervals."""

    def __init__(self, st, rays):
        self.st, self.rays = st, rays
        o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)
        self.o, self.d = o, d
        T = len(st)
        if T == 0:
            self.ray = self.tri = np.zeros(0, np.int64)
            self.t = self.u = self.v = self.det = np.zeros(0)
            self.start = np.zeros(len(rays) + 1, np.int64)
            return
        # prefilter: the ray's LINE passes the triangle's bounding sphere (about the centroid, padded for the enlarged triangle and the
        # cancellation in the expanded squares): |w|^2 - (w.d)^2 / |d|^2 <= r^2 with w = c - o, as two matrix products
        c = st.V.mean(1)
        r = np.linalg.norm(st.V - c[:, None], axis=2).max(1) * (1.0 + 4.0 * DELTA) + 1e-6 * max(st.radius, 1.0)
        dd = (d * d).sum(1)
        wd = d @ c.T - (o * d).sum(1)[:, None]
        ww = (c * c).sum(1)[None] - 2.0 * (o @ c.T) + (o * o).sum(1)[:, None]
        near = ww - wd * wd / dd[:, None] <= (r * r)[None]
        ri, ki = np.nonzero(near)  # (row-major: sorted by ray)
        D, O, e1, e2, v0 = d[ri], o[ri], st.e1[ki], st.e2[ki], st.v0[ki]
        pvec = np.cross(D, e2)
        det = (e1 * pvec).sum(1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tvec = O - v0
            u = (tvec * pvec).sum(1) * inv
            qvec = np.cross(tvec, e1)
            v = (D * qvec).sum(1) * inv
            t = (e2 * qvec).sum(1) * inv
            keep = np.isfinite(t) & (det != 0) & (np.minimum(np.minimum(u, v), 1.0 - u - v) >= -DELTA)
        self.ray, self.tri, self.t, self.u, self.v, self.det = ri[keep], ki[keep], t[keep], u[keep], v[keep], det[keep]
        self.start = np.searchsorted(self.ray, np.arange(len(rays) + 1))


class Reference:
    """The float64 closest hit of every ray in its open interval (tmin / tmax: per ray or scalars, default the rays' own), with the rays a float32
    walk may answer differently marked ambiguous:
      - the nearest hit lies within DELTA (barycentric units) of an edge, or within DELTA x max(1, t) of an end of the interval;
      - another triangle, DELTA-enlarged, is hit in front of it or within DELTA x max(1, t) behind it;
      - nothing is hit exactly but a DELTA-enlarged triangle is.
    An ambiguous ray may return any DELTA-enlarged triangle no further than DELTA x max(1, t) behind the nearest DELTA-shrunk hit, or miss when
    no DELTA-shrunk triangle is hit."""

    def __init__(self, pairs, tmin=None, tmax=None):
        st, rays = pairs.st, pairs.rays
        n = len(rays)
        o, d = pairs.o, pairs.d
        tmin = np.broadcast_to(np.maximum(rays["tMin"].astype(np.float64) if tmin is None else np.asarray(tmin, np.float64), 0.0), (n,))
        tmax = np.broadcast_to(rays["tMax"].astype(np.float64) if tmax is None else np.asarray(tmax, np.float64), (n,))
        self.tri = np.full(n, -1)  # nearest triangle hit exactly, -1 = none
        self.t = np.full(n, np.inf)
        self.u, self.v, self.det = np.zeros(n), np.zeros(n), np.zeros(n)
        self.ambiguous = np.zeros(n, bool)
        self.allowed = [None] * n  # ambiguous rays: the triangles a float32 walk may return
        self.may_miss = np.ones(n, bool)
        lo_, hi_ = tmin[pairs.ray], tmax[pairs.ray]
        margin = np.minimum(np.minimum(pairs.u, pairs.v), 1.0 - pairs.u - pairs.v)
        pad = DELTA * np.maximum(1.0, np.abs(pairs.t))
        exact = (margin >= 0) & (pairs.t > lo_) & (pairs.t < hi_)
        large = (pairs.t > lo_ - pad) & (pairs.t < hi_ + pad)
        small = (margin >= DELTA) & (pairs.t > lo_ + pad) & (pairs.t < hi_ - pad)
        for i in range(n):
            a, b = pairs.start[i], pairs.start[i + 1]
            if a == b:
                continue
            t, ex, la, sm = pairs.t[a:b], exact[a:b], large[a:b], small[a:b]
            if ex.any():
                j = int(np.where(ex, t, np.inf).argmin())
                self.tri[i], self.t[i], self.u[i], self.v[i], self.det[i] = pairs.tri[a + j], t[j], pairs.u[a + j], pairs.v[a + j], pairs.det[a + j]
                rivals = la & (t <= t[j] + DELTA * max(1.0, t[j]))
                rivals[j] = False
                amb = bool(rivals.any()) or not sm[j]
            else:
                amb = bool(la.any())
            self.may_miss[i] = not ex.any()
            if amb:
                ts = np.where(sm, t, np.inf).min()
                lim = ts + DELTA * max(1.0, ts) if np.isfinite(ts) else np.inf
                self.ambiguous[i] = True
                self.allowed[i] = set(pairs.tri[a:b][la & (t <= lim)].tolist())
                self.may_miss[i] = not np.isfinite(ts)
        self.hit = self.tri >= 0
        safe = np.maximum(self.tri, 0)
        self.position = o + np.where(self.hit, self.t, 0.0)[:, None] * d
        if len(st):
            nrm = np.cross(st.e1[safe], st.e2[safe])
            nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
            self.normal = np.where(((nrm * d).sum(1) > 0)[:, None], -nrm, nrm)
            # the world-space winding faces the ray (det > 0), inverted for a mirroring node matrix
            self.front = (self.det > 0) != st.flip[safe]
        else:
            self.normal, self.front = np.zeros((n, 3)), np.zeros(n, bool)


def check_hits(st, rays, ref, hits, tol_t, tol_b, what="", position_rounding=0.0):
    """The GPU (or host-shim) records of CLOSEST mode against the reference: exact ids on unambiguous rays within the tolerances, the allowed
    sets on ambiguous ones.  Returns the largest errors seen (t relative to max(1, t), barycentrics, position, normal).
    position_rounding: what the float32 rounding of a hit position itself may add to its error (half an ulp of the largest coordinate: for scenes
    far from the origin, where that exceeds the share of t's tolerance)."""
    HIT, FRONT, INVALID = 1, 2, 4
    assert not (hits["flags"] & INVALID).any(), what
    got_hit = (hits["flags"] & HIT) != 0
    assert ((hits["renderNode"] >= 0) == got_hit).all(), what
    miss = hits[~got_hit]
    assert (miss["renderNode"] == -1).all() and (miss["flags"] == 0).all(), what
    z = miss.copy()
    z["renderNode"] = 0
    assert not z.view(np.uint8).any(), (what, "a miss record holds something")
    # ambiguous rays
    key = {}
    for i in np.nonzero(ref.ambiguous)[0]:
        if not got_hit[i]:
            assert ref.may_miss[i], (what, "ambiguous ray", int(i), "missed although a shrunk triangle is hit")
            continue
        if not key:
            key = {(int(a), int(b)): j for j, (a, b) in enumerate(zip(st.node, st.tri))}
        j = key.get((int(hits["renderNode"][i]), int(hits["triangle"][i])), -1)
        assert j in ref.allowed[i], (what, "ambiguous ray", int(i), "returned a triangle outside its candidates", j, ref.allowed[i])
    # every other ray
    s = ~ref.ambiguous
    assert (got_hit[s] == ref.hit[s]).all(), (what, "hit / miss differs on", np.nonzero(s & (got_hit != ref.hit))[0][:8])
    h = s & ref.hit
    k = ref.tri[h]
    for name, want in (("renderNode", st.node[k]), ("renderPrimID", st.prim[k]), ("triangle", st.tri[k]), ("materialID", st.mat[k])):
        bad = hits[name][h].astype(np.int64) != want
        assert not bad.any(), (what, name, int(bad.sum()), np.nonzero(h)[0][bad][:8], hits[name][h][bad][:8], want[bad][:8])
    g = hits[h]
    err_t = np.abs(g["t"].astype(np.float64) - ref.t[h]) / np.maximum(1.0, ref.t[h])
    err_b = np.maximum(np.abs(g["b1"].astype(np.float64) - ref.u[h]), np.abs(g["b2"].astype(np.float64) - ref.v[h]))
    err_p = np.abs(g["position"].astype(np.float64) - ref.position[h]).max(1)
    err_n = np.abs(g["normal"].astype(np.float64) - ref.normal[h]).max(1)
    out = {k_: float(v.max()) if len(v) else 0.0 for k_, v in (("t", err_t), ("b", err_b), ("position", err_p), ("normal", err_n))}
    print("QUERY", what, "rays", len(rays), "hits", int(h.sum()), "ambiguous", int(ref.ambiguous.sum()), "errors", out, "tolerances", tol_t, tol_b,
          "size", st.size)
    assert out["t"] <= tol_t and out["b"] <= tol_b, (what, out)
    assert out["position"] <= tol_t * max(1.0, st.size) + position_rounding and out["normal"] <= tol_t * max(1.0, st.size), (what, out, st.size)
    assert (np.abs(np.linalg.norm(g["normal"].astype(np.float64), axis=1) - 1.0) < 1e-6).all(), what
    # (the device turns the normal by ITS dot product, a chain of fmas; another summation order may land a last-place unit above zero on a grazing ray)
    assert ((g["normal"].astype(np.float64) * rays["direction"][h].astype(np.float64)).sum(1) <= 1e-7).all(), what
    assert (((g["flags"] & FRONT) != 0) == ref.front[h]).all(), (what, "front-face bit")
    return out
