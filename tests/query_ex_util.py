"""Shared helpers of the tests of the _ex ray queries (mi_pt_query_rays_ex & co.: alpha-aware, face-culled, K nearest), next to tests/query_util.py
whose SceneTris, Pairs, DELTA and check_hits they reuse: the alpha side of a scene description in float64 (SceneAlpha), the exact STOCHASTIC draw,
the float64 reference of the new semantics with its ambiguity classes (ReferenceEx), the check of K-lists, the device's alpha records as arrays
and the host shim that runs the device's per-ray code over them (tests/host_shim/query_ex_on_host.cpp).  No GPU needed.

Ambiguity.  A candidate (ray, triangle) is alpha-ambiguous when its float64 opacity lies within ALPHA_BAND of the value it is compared with (the
material's cutoff under MASK, the caller's threshold or the draw under BLEND), or when the decision differs at one of the four barycentric points
displaced by +-DELTA (a texel boundary, a steep vertex-alpha gradient).  ALPHA_BAND = 1e-5: the float32 opacity is at most about a dozen roundings
of values <= 1, under 1e-6; the band is ten times that.  A candidate is cull-ambiguous when the ray grazes its plane (|cos| < 1e-5: the sign of
the determinant is the facing).  A ray is ambiguous if the geometric rule of query_util.Reference says so over the accepted set, or an
ambiguous candidate lies at or in front of the answer; it may then return whatever flipping the ambiguous decisions allows."""
import ctypes as C
import os
import subprocess

import numpy as np

import query_util as qu
from query_util import DELTA, F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA_BAND = 1e-5
GRAZING = 1e-5
CLOSEST, ANY, NEAREST_K = 0, 1, 2
OPAQUE, CUTOFF, STOCHASTIC = 0, 1, 2
CULL_NONE, CULL_MATERIAL = 0, 1
INST_FORCE_OPAQUE, INST_CULL_DISABLE, INST_FLIP_FACING, INST_TRANSMISSIVE, INST_ALPHA_PASSES = 1, 2, 4, 8, 16
ALPHA_OPAQUE, ALPHA_MASK, ALPHA_BLEND = 0, 1, 2
WRAP_REPEAT, WRAP_CLAMP, WRAP_MIRROR = 0, 1, 2
AT_HAS_TEXTURE, AT_LINEAR, AT_WRAPS_SHIFT, AT_WRAPT_SHIFT, AT_HAS_COLORS = 1 << 2, 1 << 3, 4, 6, 1 << 8  # pt_scene.h
# DevAlphaTri (pt_scene.h), QueryRules (pt_query.h)
ALPHA_DTYPE = np.dtype([("uv0", "<f4", (2,)), ("uv1", "<f4", (2,)), ("uv2", "<f4", (2,)), ("factor", "<f4"), ("cutoff", "<f4"), ("texel", "<u4"),
                        ("size", "<u4"), ("flags", "<u4"), ("colors", "<u4")])
RULES_DTYPE = np.dtype([("alpha", "<i4"), ("cull", "<i4"), ("maxHits", "<i4"), ("blendThreshold", "<f4"), ("seed", "<u4")])
assert ALPHA_DTYPE.itemsize == 48 and RULES_DTYPE.itemsize == 20

# The scenes of the reference comparison.  The first two are query_util's (its TOLERANCE holds); for the two zoo scenes the pair below is MEASURED
# the way query_util.measure_float32_error measures (float32 ray / triangle test against float64 on the unambiguous opaque closest hits of
# make_rays_ex), and the tolerance is 8 x it -- the margin and its reason are query_util's (the one rounding the device adds when it forms the
# world-space edges).  tests/test_query_ex_reference.py re-measures.
SCENES = ("mixed_alpha_glass", "zoo_blend", "zoo_vertex_streams", "atrium_sliver")
MEASURED = {
    "zoo_blend": (1.0874e-06, 7.6392e-05),
    "zoo_vertex_streams": (1.0097e-06, 1.00991e-04),
}
TOLERANCE = {k: (8.0 * t, 8.0 * b) for k, (t, b) in MEASURED.items()}
TOLERANCE.update({k: qu.TOLERANCE[k] for k in ("mixed_alpha_glass", "atrium_sliver")})
MAX_AMBIGUOUS_SHARE = 0.02  # (rays aimed at triangles graze more edges than rays aimed at the bounds: query_util's 1 % does not carry over)
MIN_OUTCOME_SHARE = 0.05    # both alpha outcomes occur on at least this share of the rays


def make_scene(name, directory):
    from vk_gltf_renderer_amd import scenegen
    path = os.path.join(str(directory), name + ".glb")
    if name == "zoo_blend":
        return scenegen.scene_material_zoo(path, "blend")
    if name == "zoo_vertex_streams":
        return scenegen.scene_material_zoo(path, "vertex_streams")
    return qu.make_scene(name, directory)


# ---- the alpha side of a scene description ------------------------------------------------------------------------------------------------------
def material_inst_flags(mat):
    """materialInstFlags (mi_pt_api.hip)."""
    f = 0
    if mat.transmissionFactor == 0.0 and mat.alphaMode == ALPHA_OPAQUE and mat.diffuseTransmissionFactor == 0.0:
        f |= INST_FORCE_OPAQUE
    if mat.doubleSided == 1 or mat.thicknessFactor > 0.0 or mat.transmissionFactor > 0.0:
        f |= INST_CULL_DISABLE
    if mat.transmissionFactor > F32(0.01):
        f |= INST_TRANSMISSIVE
    if not (f & INST_FORCE_OPAQUE) and mat.alphaMode == ALPHA_OPAQUE:
        f |= INST_ALPHA_PASSES
    return f


class SceneAlpha:
    """Per triangle of a query_util.SceneTris (same order): the instance flags of its triangle record, and what makeAlphaRecord (pt_shading.h) reads
    of the description -- alpha mode, factor and cutoff, the level-0 alpha texels with their sampler, the three uvs of the set the texture uses, the
    vertex-colour alphas."""

    def __init__(self, scene, st):
        d = scene.desc.contents
        flags, mode, factor, cutoff, tex, uv, va, has_va = [], [], [], [], [], [], [], []
        self.textures = {}
        for n in range(d.numRenderNodes):
            rn = d.renderNodes[n]
            if d.renderNodeVisible and not d.renderNodeVisible[n]:
                continue
            if rn.renderPrimID < 0 or rn.renderPrimID >= d.numRenderPrimitives:
                continue
            rp = d.renderPrimitives[rn.renderPrimID]
            k = int(rp.triangleCount)
            if k == 0:
                continue
            mat = d.materials[max(0, rn.materialID)]
            f = material_inst_flags(mat)
            M = np.array(rn.objectToWorld[:], np.float64).reshape(4, 4).T
            if np.linalg.det(M[:3, :3]) < 0:
                f |= INST_FLIP_FACING
            fl = np.full(k, f)
            fl[:int(rp.opaqueTriangleCount)] |= INST_FORCE_OPAQUE
            flags.append(fl)
            idx = np.ctypeslib.as_array(rp.indices, shape=(k, 3)).astype(np.int64)
            sg = mat.pbrModel == 1  # MI_PBR_SPECULAR_GLOSSINESS
            mode.append(np.full(k, mat.alphaMode))
            factor.append(np.full(k, F32(mat.pbrDiffuseFactor[3] if sg else mat.pbrBaseColorFactor[3]), F32))
            cutoff.append(np.full(k, F32(mat.alphaCutoff), F32))
            t_id, t_uv = -1, np.zeros((k, 3, 2), F32)
            slot = mat.pbrDiffuseTexture if sg else mat.pbrBaseColorTexture
            if mat.alphaMode != ALPHA_OPAQUE and slot > 0:
                info = d.textureInfos[slot]
                if 0 <= info.index < d.numTextures:
                    t_id = int(info.index)
                    self._texture(d, t_id)
                    tc = rp.texCoords0 if info.texCoord == 0 else rp.texCoords1
                    if tc:
                        t_uv = np.ctypeslib.as_array(tc, shape=(rp.vertexCount, 2))[idx].astype(F32)
            tex.append(np.full(k, t_id))
            uv.append(t_uv)
            if rp.colors and mat.alphaMode != ALPHA_OPAQUE:
                va.append((np.ctypeslib.as_array(rp.colors, shape=(rp.vertexCount,))[idx] >> 24).astype(np.int64))
                has_va.append(np.ones(k, bool))
            else:
                va.append(np.zeros((k, 3), np.int64))
                has_va.append(np.zeros(k, bool))
        cat = lambda parts, dt, shape: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
        self.flags, self.mode, self.tex = (cat(x, np.int64, (0,)) for x in (flags, mode, tex))
        self.factor, self.cutoff = cat(factor, F32, (0,)), cat(cutoff, F32, (0,))
        self.uv, self.va, self.has_va = cat(uv, F32, (0, 3, 2)), cat(va, np.int64, (0, 3)), cat(has_va, bool, (0,))
        assert len(self.flags) == len(st)
        self.tested = (self.flags & (INST_FORCE_OPAQUE | INST_ALPHA_PASSES)) == 0  # the triangles an alpha-aware walk tests
        assert (self.mode[self.tested] != ALPHA_OPAQUE).all()

    def _texture(self, d, t_id):
        if t_id in self.textures:
            return
        t = d.textures[t_id]
        rgba = np.ctypeslib.as_array(t.levels[0], shape=(t.height, t.width, 4)).copy()
        self.textures[t_id] = dict(rgba=rgba, w=int(t.width), h=int(t.height), wrapS=int(t.wrapS), wrapT=int(t.wrapT), linear=int(t.magFilter) == 1)

    @staticmethod
    def _wrap(i, n, mode):
        if mode == WRAP_CLAMP:
            return np.clip(i, 0, n - 1)
        if mode == WRAP_MIRROR:
            m = np.mod(i, 2 * n)
            return np.where(m < n, m, 2 * n - 1 - m)
        return np.mod(i, n)

    def _sample(self, t, x, y):
        """Level-0 alpha at uv (x, y): nearest or bilinear by the magnification filter, no UV transform (as the frames' alpha test)."""
        a = t["rgba"][:, :, 3].astype(np.float64) / 255.0
        fx, fy = x * t["w"], y * t["h"]
        if not t["linear"]:
            return a[self._wrap(np.floor(fy).astype(np.int64), t["h"], t["wrapT"]), self._wrap(np.floor(fx).astype(np.int64), t["w"], t["wrapS"])]
        fx, fy = fx - 0.5, fy - 0.5
        ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        tx, ty = fx - ix, fy - iy
        x0, x1 = self._wrap(ix, t["w"], t["wrapS"]), self._wrap(ix + 1, t["w"], t["wrapS"])
        y0, y1 = self._wrap(iy, t["h"], t["wrapT"]), self._wrap(iy + 1, t["h"], t["wrapT"])
        return (a[y0, x0] * (1 - tx) + a[y0, x1] * tx) * (1 - ty) + (a[y1, x0] * (1 - tx) + a[y1, x1] * tx) * ty

    def alpha(self, k, u, v):
        """The float64 alpha of triangles k at barycentrics (u, v) BEFORE the MASK cutoff: factor x texel x vertex alpha."""
        k, u, v = np.asarray(k), np.asarray(u, np.float64), np.asarray(v, np.float64)
        b0 = 1.0 - u - v
        a = self.factor[k].astype(np.float64)
        uv = self.uv[k].astype(np.float64)
        for t_id, t in self.textures.items():
            s = self.tex[k] == t_id
            if s.any():
                x = uv[s, 0, 0] * b0[s] + uv[s, 1, 0] * u[s] + uv[s, 2, 0] * v[s]
                y = uv[s, 0, 1] * b0[s] + uv[s, 1, 1] * u[s] + uv[s, 2, 1] * v[s]
                a[s] *= self._sample(t, x, y)
        va = self.va[k] / 255.0
        return np.where(self.has_va[k], a * (va[:, 0] * b0 + va[:, 1] * u + va[:, 2] * v), a)

    def device_records(self):
        """(DevAlphaTri array, texel pool as (n, 4) uint8): what makeAlphaRecord writes, one slot per triangle, level 0 of each texture pooled."""
        rec = np.zeros(len(self.flags), ALPHA_DTYPE)
        rec["factor"], rec["cutoff"] = 1.0, 0.5
        pool, offset = [], {}
        for t_id, t in self.textures.items():
            offset[t_id] = sum(len(p) for p in pool)
            pool.append(t["rgba"].reshape(-1, 4))
        live = self.mode != ALPHA_OPAQUE
        rec["factor"][live], rec["cutoff"][live] = self.factor[live], self.cutoff[live]
        fl = self.mode.copy()
        for t_id, t in self.textures.items():
            s = live & (self.tex == t_id)
            rec["uv0"][s], rec["uv1"][s], rec["uv2"][s] = self.uv[s, 0], self.uv[s, 1], self.uv[s, 2]
            rec["texel"][s], rec["size"][s] = offset[t_id], t["w"] | (t["h"] << 16)
            fl[s] |= AT_HAS_TEXTURE | (AT_LINEAR if t["linear"] else 0) | (t["wrapS"] << AT_WRAPS_SHIFT) | (t["wrapT"] << AT_WRAPT_SHIFT)
        c = live & self.has_va
        fl[c] |= AT_HAS_COLORS
        rec["colors"][c] = self.va[c, 0] | (self.va[c, 1] << 8) | (self.va[c, 2] << 16)
        rec["flags"] = np.where(live, fl, 0)
        texels = np.ascontiguousarray(np.concatenate(pool)) if pool else np.zeros((1, 4), np.uint8)
        return rec, texels


# ---- the STOCHASTIC draw, exactly ---------------------------------------------------------------------------------------------------------------
def xxhash32(px, py, pz):
    """pt_math.h: xxhash32, on arrays (uint64 arithmetic masked to 32 bits: a product of two 32-bit values fits)."""
    M = np.uint64(0xffffffff)
    P2, P3, P4, P5 = (np.uint64(x) for x in (2246822519, 3266489917, 668265263, 374761393))
    px, py, pz = (np.asarray(x).astype(np.uint64) & M for x in (px, py, pz))
    rot = lambda h: ((h << np.uint64(17)) | (h >> np.uint64(15))) & M
    h = (pz + P5 + ((px * P3) & M)) & M
    h = (P4 * rot(h)) & M
    h = (h + ((py * P3) & M)) & M
    h = (P4 * rot(h)) & M
    h = (P2 * (h ^ (h >> np.uint64(15)))) & M
    h = (P3 * (h ^ (h >> np.uint64(13)))) & M
    return h ^ (h >> np.uint64(16))


def draw(seed, ray_index, rnode, prim):
    """candidateRand(xxhash32(seed, i, 0), renderNode, triangle): u32ToUnitFloat keeps the top 23 bits -- (h >> 9) / 2^23, exact in float32."""
    return (xxhash32(xxhash32(seed, ray_index, 0), rnode, prim) >> np.uint64(9)).astype(np.float64) / 8388608.0


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------------
GRAZE_MIN = 0.05


def make_rays_ex(st, sa, n=1024, seed=7):
    """query_util.make_rays(st, n, seed), then n rays from the sphere of 1.5 x the bounds' radius aimed at uniform points of uniformly chosen
    triangles whose material is not alphaMode OPAQUE (so that alpha decisions are met in numbers).
    The aimed rays are the first n of 2 n drawn that graze nothing: no DELTA-enlarged triangle along the ray's line meets it at |cos| < GRAZE_MIN
    to its normal.  Why: the float32 ray / triangle test divides by the determinant, which is proportional to that cosine; measured as
    query_util.measure_float32_error measures (float32 test against float64, mixed alpha + glass scene, rays aimed like these), the barycentric
    error is about 2e-6 / |cos| -- 1.0e-4 at 0.020, 1.8e-4 at 0.0064, 7.1e-4 at 0.0023 -- so below |cos| 0.02 it exceeds DELTA and the
    reference's DELTA classes no longer bound what float32 may answer (a ray along a sphere's silhouette is outside both triangles at the fold
    by float64 and inside one by float32).  At 0.05 it is 4e-5.  Rays aimed at the bounds meet such triangles an order of magnitude less often
    than rays aimed at geometry; query_util's recipe, the first half, stays as it is."""
    rays = qu.make_rays(st, n, seed)
    area = np.linalg.norm(np.cross(st.e1, st.e2), axis=1)
    # (not the degenerate triangles at a sphere's poles: every point of one lies on an edge of its neighbours)
    pool = np.nonzero((sa.mode != ALPHA_OPAQUE) & (area > 1e-6 * np.median(area)))[0] if len(st) else []
    if len(pool) == 0:
        return rays
    rng = np.random.default_rng(seed + 1000)
    m = 2 * n
    c = 0.5 * (st.lo + st.hi)
    o = rng.normal(size=(m, 3))
    o = c + 1.5 * st.radius * o / np.linalg.norm(o, axis=1, keepdims=True)
    k = pool[rng.integers(0, len(pool), m)]
    r1, r2 = np.sqrt(rng.uniform(size=m)), rng.uniform(size=m)
    p = st.V[k, 0] * (1 - r1)[:, None] + st.V[k, 1] * (r1 * (1 - r2))[:, None] + st.V[k, 2] * (r1 * r2)[:, None]
    dd = p - o
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    aimed = np.zeros(m, qu.RAY_DTYPE)
    aimed["origin"], aimed["direction"], aimed["tMin"], aimed["tMax"] = o, dd, 0.0, np.inf
    pairs = qu.Pairs(st, aimed)
    cos = np.abs(pairs.det) / np.maximum(np.linalg.norm(np.cross(st.e1[pairs.tri], st.e2[pairs.tri]), axis=1) * np.linalg.norm(pairs.d[pairs.ray], axis=1), 1e-300)
    grazes = np.bincount(pairs.ray[cos < GRAZE_MIN], minlength=m) > 0
    keep = np.nonzero(~grazes)[0][:n]
    assert len(keep) == n, (len(keep), "of", m, "drawn rays graze nothing")
    return np.concatenate([rays, aimed[keep]])


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------------------
class Decisions:
    """Per pair of a query_util.Pairs, under (alpha, cull, blend_threshold, seed): `sure` -- accepted, and no float32 evaluation may say otherwise;
    `maybe` -- ambiguous, and not surely rejected by the other test; `nominal` -- what float64 says.  Ray indices are the rays' positions in the
    call (the draw is keyed on them)."""

    def __init__(self, pairs, sa, alpha=OPAQUE, cull=CULL_NONE, blend_threshold=0.5, seed=0):
        st, k = pairs.st, pairs.tri
        n = len(k)
        yes, no = np.ones(n, bool), np.zeros(n, bool)
        # culling: the object-space facing is the sign of the determinant, inverted by a mirroring matrix
        if cull == CULL_NONE or n == 0:
            c_pass, c_amb = yes, no
        else:
            front = (pairs.det > 0) != st.flip[k]
            c_pass = front | ((sa.flags[k] & INST_CULL_DISABLE) != 0)
            nrm = np.cross(st.e1[k], st.e2[k])
            cos = np.abs(pairs.det) / np.maximum(np.linalg.norm(nrm, axis=1) * np.linalg.norm(pairs.d[pairs.ray], axis=1), 1e-300)
            c_amb = (cos < GRAZING) & ((sa.flags[k] & INST_CULL_DISABLE) == 0)
        # alpha
        self.tested = (sa.tested[k] if n else no) & (alpha != OPAQUE)
        a_pass, a_amb = yes.copy(), no.copy()
        self.alpha_value = np.ones(n)
        s = np.nonzero(self.tested)[0]
        if len(s):
            ks, u, v = k[s], pairs.u[s], pairs.v[s]
            mask = sa.mode[ks] == ALPHA_MASK
            dr = draw(seed, pairs.ray[s], st.node[ks], st.tri[ks]) if alpha == STOCHASTIC else np.zeros(len(s))
            value = np.where(mask, sa.cutoff[ks].astype(np.float64), float(F32(blend_threshold)) if alpha == CUTOFF else dr)

            def decide(uu, vv):
                raw = sa.alpha(ks, uu, vv)
                if alpha == CUTOFF:
                    return raw, raw >= value  # (MASK: o = [raw >= cutoff], and o >= threshold for every threshold in (0, 1])
                o = np.where(mask, (raw >= value).astype(np.float64), raw)
                return raw, dr <= o

            raw, ok = decide(u, v)
            amb = np.abs(raw - value) < ALPHA_BAND
            for du, dv in ((DELTA, 0), (-DELTA, 0), (0, DELTA), (0, -DELTA)):
                amb |= decide(u + du, v + dv)[1] != ok
            a_pass[s], a_amb[s], self.alpha_value[s] = ok, amb, raw
        self.nominal = c_pass & a_pass
        self.sure = (c_pass & ~c_amb) & (a_pass & ~a_amb)
        self.maybe = (c_pass | c_amb) & (a_pass | a_amb) & ~self.sure
        self.alpha_ambiguous = a_amb & (c_pass | c_amb)
        self.rejected_by_alpha = self.tested & ~a_pass


class ReferenceEx:
    """query_util.Reference over the accepted set, with the attributes query_util.check_hits reads.  Per pair: `ex` (hit exactly, accepted by
    float64), `la` (DELTA-enlarged, accepted or ambiguous), `sm` (DELTA-shrunk and surely accepted)."""

    def __init__(self, pairs, dec, tmin=None, tmax=None):
        st, rays = pairs.st, pairs.rays
        n = len(rays)
        o, d = pairs.o, pairs.d
        tmin = np.broadcast_to(np.maximum(rays["tMin"].astype(np.float64) if tmin is None else np.asarray(tmin, np.float64), 0.0), (n,))
        tmax = np.broadcast_to(rays["tMax"].astype(np.float64) if tmax is None else np.asarray(tmax, np.float64), (n,))
        self.pairs, self.dec = pairs, dec
        self.tri = np.full(n, -1)
        self.t = np.full(n, np.inf)
        self.u, self.v, self.det = np.zeros(n), np.zeros(n), np.zeros(n)
        self.ambiguous = np.zeros(n, bool)
        self.alpha_only = np.zeros(n, bool)  # ambiguous, and the geometric rule over float64's accepted set alone would not say so
        self.allowed = [None] * n
        self.may_miss = np.ones(n, bool)
        lo_, hi_ = tmin[pairs.ray], tmax[pairs.ray]
        margin = np.minimum(np.minimum(pairs.u, pairs.v), 1.0 - pairs.u - pairs.v)
        pad = DELTA * np.maximum(1.0, np.abs(pairs.t))
        inside = (pairs.t > lo_ - pad) & (pairs.t < hi_ + pad)
        self.ex = (margin >= 0) & (pairs.t > lo_) & (pairs.t < hi_) & dec.nominal
        self.la = inside & (dec.sure | dec.maybe)
        self.sm = (margin >= DELTA) & (pairs.t > lo_ + pad) & (pairs.t < hi_ - pad) & dec.sure
        geo_la = inside & dec.nominal
        geo_sm = (margin >= DELTA) & (pairs.t > lo_ + pad) & (pairs.t < hi_ - pad) & dec.nominal
        for i in range(n):
            a, b = pairs.start[i], pairs.start[i + 1]
            if a == b:
                continue
            t, ex, la, sm = pairs.t[a:b], self.ex[a:b], self.la[a:b], self.sm[a:b]
            if ex.any():
                j = int(np.where(ex, t, np.inf).argmin())
                self.tri[i], self.t[i], self.u[i], self.v[i], self.det[i] = pairs.tri[a + j], t[j], pairs.u[a + j], pairs.v[a + j], pairs.det[a + j]
                lim_j = t[j] + DELTA * max(1.0, t[j])
                rivals = la & (t <= lim_j)
                rivals[j] = False
                amb = bool(rivals.any()) or not sm[j]
                grivals = geo_la[a:b] & (t <= lim_j)
                grivals[j] = False
                geo = bool(grivals.any()) or not geo_sm[a + j]
            else:
                amb = bool(la.any())
                geo = bool(geo_la[a:b].any())
            self.may_miss[i] = not ex.any()
            if amb:
                ts = np.where(sm, t, np.inf).min()
                lim = ts + DELTA * max(1.0, ts) if np.isfinite(ts) else np.inf
                self.ambiguous[i] = True
                self.alpha_only[i] = not geo
                self.allowed[i] = set(pairs.tri[a:b][la & (t <= lim)].tolist())
                self.may_miss[i] = not np.isfinite(ts)
        self.hit = self.tri >= 0
        safe = np.maximum(self.tri, 0)
        self.position = o + np.where(self.hit, self.t, 0.0)[:, None] * d
        if len(st):
            nrm = np.cross(st.e1[safe], st.e2[safe])
            nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
            self.normal = np.where(((nrm * d).sum(1) > 0)[:, None], -nrm, nrm)
            self.front = (self.det > 0) != st.flip[safe]
        else:
            self.normal, self.front = np.zeros((n, 3)), np.zeros(n, bool)

    def outcome_shares(self):
        """(share of rays with >= 1 candidate the alpha test rejects, share with >= 1 tested candidate it accepts) -- candidates hit exactly inside
        the ray's interval, in float64."""
        p, n = self.pairs, len(self.pairs.rays)
        margin = np.minimum(np.minimum(p.u, p.v), 1.0 - p.u - p.v)
        live = (margin >= 0) & (p.t > 0)
        rej = np.bincount(p.ray[live & self.dec.rejected_by_alpha], minlength=n) > 0
        acc = np.bincount(p.ray[live & self.dec.tested & ~self.dec.rejected_by_alpha], minlength=n) > 0
        return float(rej.mean()), float(acc.mean())


def check_lists(st, rays, ref, lists, k, tol_t, what=""):
    """(n, k) NEAREST_K records against a ReferenceEx, ray by ray, without an exclusion class: every returned record is a DELTA-enlarged accepted
    (or ambiguous) hit with its t within tolerance; t does not decrease; no (renderNode, triangle) repeats; every unambiguous accepted hit nearer
    than the last returned t minus the pad is present (every one, when the list is not full); the count lies between the numbers of DELTA-shrunk
    and DELTA-enlarged accepted hits, capped at k; unused records are miss records at the end."""
    HIT, INVALID = 1, 4
    p = ref.pairs
    assert lists.shape == (len(rays), k), (what, lists.shape)
    assert not (lists["flags"] & INVALID).any(), what
    got = (lists["flags"] & HIT) != 0
    assert (got[:, :-1] | ~got[:, 1:]).all(), (what, "a hit follows a miss record")
    miss = lists[~got].copy()
    assert (miss["renderNode"] == -1).all() and (miss["flags"] == 0).all(), what
    miss["renderNode"] = 0
    assert not miss.view(np.uint8).any(), (what, "a miss record holds something")
    key = {(int(a), int(b)): j for j, (a, b) in enumerate(zip(st.node, st.tri))}
    worst, bad = 0.0, []
    for i in range(len(rays)):
        a, b = p.start[i], p.start[i + 1]
        tri, t, la, sm = p.tri[a:b], p.t[a:b], ref.la[a:b], ref.sm[a:b]
        cnt = int(got[i].sum())
        if not min(k, int(sm.sum())) <= cnt <= min(k, int(la.sum())):
            bad.append((i, "count", cnt, int(sm.sum()), int(la.sum())))
        rec = lists[i, :cnt]
        ids = [key.get((int(r["renderNode"]), int(r["triangle"])), -1) for r in rec]
        if len(set(ids)) != cnt:
            bad.append((i, "repeats a triangle", ids))
        if not (np.diff(rec["t"]) >= 0).all():
            bad.append((i, "t decreases", rec["t"].tolist()))
        large = {int(x): float(tt) for x, tt in zip(tri[la], t[la])}
        for r, j in zip(rec, ids):
            if j not in large:
                bad.append((i, "returned a triangle outside its candidates", j))
                continue
            err = abs(float(r["t"]) - large[j]) / max(1.0, large[j])
            worst = max(worst, err)
            if err > tol_t:
                bad.append((i, "t", float(r["t"]), large[j]))
        last = float(rec["t"][-1]) if cnt == k else np.inf
        need = sm & (t < last - DELTA * np.maximum(1.0, np.abs(t)))
        missing = set(tri[need].tolist()) - set(ids)
        if missing:
            bad.append((i, "misses unambiguous hits", sorted(missing)))
    print("QUERY_EX", what, "lists of", k, "rays", len(rays), "records", int(got.sum()), "worst t error", worst, "tolerance", tol_t, "failures", len(bad))
    assert not bad, (what, len(bad), bad[:8])
    return worst


# ---- the device's per-ray code on the host --------------------------------------------------------------------------------------------------------
def rules(alpha=OPAQUE, cull=CULL_NONE, max_hits=1, blend_threshold=0.5, seed=0):
    r = np.zeros(1, RULES_DTYPE)
    r["alpha"], r["cull"], r["maxHits"], r["blendThreshold"], r["seed"] = alpha, cull, max_hits, blend_threshold, seed
    return r


class Shim:
    """tests/host_shim/query_ex_on_host.cpp, compiled into `directory`."""

    def __init__(self, directory):
        out = os.path.join(str(directory), "libquery_ex_on_host.so")
        shim = os.path.join(ROOT, "tests", "host_shim")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + shim,
                        "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"), "-I" + os.path.join(ROOT, "include"), "-o", out,
                        os.path.join(shim, "query_ex_on_host.cpp")], check=True)
        L = self.lib = C.CDLL(out)
        VP, I, F, U = C.c_void_p, C.c_int, C.c_float, C.c_uint32
        L.query_ex_layout.argtypes = [VP]
        L.query_ex_brute.argtypes = [VP, VP, VP, VP, VP, I, VP, I, I, VP, I, VP]
        L.query_ex_opacity.argtypes, L.query_ex_opacity.restype = [VP, VP, I, F, F], F
        L.query_ex_draw.argtypes, L.query_ex_draw.restype = [U, U, U, U], F
        L.query_ex_cull_passes.argtypes, L.query_ex_cull_passes.restype = [U, I, I], I
        L.query_ex_alpha_decision.argtypes, L.query_ex_alpha_decision.restype = [I, F, F, F], I

    def brute(self, tris, shade, alpha, texels, rays, r, any_hit=False, order=None, first=0):
        """Every ray against every triangle slot of `order`: (n, maxHits) records."""
        order = np.ascontiguousarray(np.arange(len(tris)) if order is None else order, np.int32)
        rays = np.ascontiguousarray(rays)
        out = np.zeros((len(rays), int(r["maxHits"][0])), qu_hit_dtype())
        self.lib.query_ex_brute(tris.ctypes.data, shade.ctypes.data, alpha.ctypes.data, texels.ctypes.data, order.ctypes.data, len(order),
                                rays.ctypes.data, len(rays), first, r.ctypes.data, int(any_hit), out.ctypes.data)
        return out


def qu_hit_dtype():
    from vk_gltf_renderer_amd import pathtracer as ptmod
    return ptmod.HIT_DTYPE


def shim_records(st, sa):
    """(DevTri, DevShadeTri, DevAlphaTri, texels) of a scene, one slot per triangle, the triangle records carrying the instance flags."""
    tris, shade = st.device_records()
    tris["flags"] = sa.flags
    alpha, texels = sa.device_records()
    return tris, shade, alpha, texels
