"""Float64 reference of the texture fetch and of the glTF material maps, for tests/test_texture_on_host.py (CPU tier) and
tests/test_gpu_texture_views.py (GPU tier).  No GPU needed.

Written from the glTF 2.0 sampler rules (section 3.8.4 / 5.26: filters, wrap modes), the level-of-detail rules glTF inherits from
OpenGL / Vulkan (Vulkan 1.3 section 16.5-16.9: level sizes max(1, W >> l), unnormalised coordinates u * w, the -0.5 shift and the
floor of a linear footprint, wrap as an integer function of the texel index, lod <= 0 is a magnification), the sRGB EOTF of IEC
61966-2-1, and the material extension specifications (KHR_materials_clearcoat, _sheen, _specular, _transmission, _iridescence,
_anisotropy, _diffuse_transmission, _pbrSpecularGlossiness, KHR_texture_transform).  It is NOT a transcription of
csrc/device/pt_shading.h.

Decisions versus values.  A fetch DECIDES which texel, which level and which weights tx, ty; the VALUES (texel decode, blends) are
float64 here.  The decisions are restated in numpy float32 where the device's float32 arithmetic is one rounding per operation:
  * unnormalised coordinate: one multiply u * float(w); a linear footprint subtracts 0.5 and floors; the weight is the exact
    difference fx - floor(fx) (exact in binary floating point);
  * the texture coordinate under a transform WITHOUT rotation (uvTransform[1] == uvTransform[2] == 0): u * sx is one multiply, the
    cross term is an exact zero, the offset one add.
Where they cannot be restated the reference computes the float64 quantity and reports every outcome whose decision boundary lies
within a band of it; a case with more than one distinct outcome is UNDECIDED and the code under test must match one of them:
  * UV_BAND = 1e-6 (in uv): the coordinate under a ROTATION is a float32 product, an fma and an add of magnitudes below 8 in the
    cases (uv magnitudes stay below 64 in any case: beyond, int(floor(u * w)) of a 16384-wide level could overflow 32 bits -- out
    of scope).  Three roundings of at most half an ulp(8) = 2^-21 each are 7.2e-7.  A NEAREST texel choice within the band of a
    texel edge has two outcomes; a LINEAR footprint is continuous across its boundary, so the band goes into the value bound
    instead (conditioning: the change of the reference under uv +- UV_BAND).
  * LOD_BAND = 1e-5 (in levels): rho = sqrt(max(ax^2 + bx^2, ay^2 + by^2)) with ax = (U0 * texGrad) * W.  On the host compile
    (IEEE, libm) the chain is 2 roundings per a, one per square, one fma, half of the sum through a correctly rounded sqrt plus its
    own: a relative 4 * 2^-24 of rho, i.e. 4 * 2^-24 / ln 2 = 3.4e-7 levels, plus log2f's last place at a result below 8 (2^-21 =
    4.8e-7): DELTA_LOD_LIBM = 8.2e-7.  On the device texGrad itself carries the hit distance, the cosine and the texel density
    (a dozen more roundings, an approximate division and square root: about 20 * 2^-24 relative = 1.7e-6 levels) and the fast log2
    one place of its result: about 2.2e-6.  The band is some four times that, and ten times below the 1e-4 ceiling of the issue.
    Boundaries: lod = 0 (magnification filter against minification filter -- two outcomes only where the two filters differ) and,
    under NEAREST level selection, lod + 0.5 integral.  Under LINEAR level selection the blend is continuous in lod; its error goes
    into the value bound as |b - a| * delta_lod (a, b: the level values of the pairs blended at or next to this lod: Outcome.spread).

Choices the specifications leave open follow the reference renderer's shaders/gltf_material_eval.h.slang (cited per line below):
the 0.0014142 roughness floor before squaring (:51, :214), the 0.001 clearcoat-roughness floor (:330), occlusion as 1 + s (R - 1)
(:226), the tangent frame update after a normal map or an anisotropy direction (:400-407), iridescence off where the thickness is
0 (:357), the specular-glossiness conversion (:136-161), and -- src/gltf_scene_vk.cpp:1127-1144 -- the diffuse-transmission colour
texture decoded as the texture record says (the renderer does not mark it sRGB), not as the extension text says.
"""
import math

import numpy as np

F32 = np.float32
NEAREST, LINEAR = 0, 1
REPEAT, CLAMP, MIRROR = 0, 1, 2
UV_BAND = 1e-6
LOD_BAND = 1e-5
DELTA_LOD_LIBM = 4 * 2.0 ** -24 / math.log(2.0) + 2.0 ** -21
# Value bound of a fetch without a level blend, absolute, for texel values <= 1, in units of u = 2^-24 (one rounding of a value <= 1 is at most u/2 below 1
# and u at 1; u is used throughout): the sRGB table entry is float32 (c = i / 255: 1; + 0.055f: 1 and the constant's own 1; / 1.055f: 1 and the constant's 1 --
# a relative 5 u, times the exponent 2.4 = 12 u, plus the float32 pow's last place 2 u) 14 u; the linear decode is 2 u (the rounded 1 / 255 and the product);
# the bilinear blend 6 u (1 - tx and 1 - ty, and per pinned lerp one product and one fma, twice nested); the level blend 3 u more (1 - f, a product, an fma).
U = 2.0 ** -24
FETCH_BOUND = (14 + 6) * U            # 1.19e-6
TRILINEAR_EXTRA = 3 * U
FACTOR_ROUNDINGS = 2 * U              # a factor and a vertex colour multiplied on
OETF_SLOPE = 12.92
OETF_ABS = (2 * 1.055 + 1) * U        # tests/test_gpu_device_kat.py: 2 ulp of pow through the fma (x 1.055) plus the result's rounding, at values <= 1


class Tex:
    """A texture record: levels[l] is a (h_l, w_l, 4) uint8 array."""

    def __init__(self, levels, srgb, mag, min_, mip, wrap_s, wrap_t):
        self.levels = [np.ascontiguousarray(lv, np.uint8) for lv in levels]
        self.height, self.width = self.levels[0].shape[:2]
        self.decoded = {}
        self.srgb, self.mag, self.min, self.mip, self.wrap_s, self.wrap_t = bool(srgb), int(mag), int(min_), int(mip), int(wrap_s), int(wrap_t)
        for l, lv in enumerate(self.levels):
            assert lv.shape == (max(1, self.height >> l), max(1, self.width >> l), 4), (l, lv.shape)


def tex_from_desc(t):
    """The record of a host scene's texture (scene.desc.contents.textures[i], MiPtTexture): the mip chain is the loader's."""
    levels = [np.ctypeslib.as_array(t.levels[l], shape=(max(1, t.height >> l), max(1, t.width >> l), 4)).copy() for l in range(t.numLevels)]
    return Tex(levels, t.srgb, t.magFilter, t.minFilter, t.mipmapMode, t.wrapS, t.wrapT)


def srgb_eotf(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, np.power((c + 0.055) / 1.055, 2.4))


def srgb_oetf(c):
    c = np.asarray(c, np.float64)
    return np.where(c > 0.0031308, 1.055 * np.power(np.maximum(c, 0.0), 1.0 / 2.4) - 0.055, c * 12.92)


def wrap(i, n, mode):
    """Texel index under a wrap mode (Vulkan 16.6 "wrapping operation")."""
    if mode == CLAMP:
        return min(max(i, 0), n - 1)
    if mode == MIRROR:
        a = (i % (2 * n)) - n
        return (n - 1) - (a if a >= 0 else -(1 + a))
    return i % n


def texel(tex, level, x, y):
    if level not in tex.decoded:
        p = tex.levels[level].astype(np.float64) / 255.0
        if tex.srgb:
            p[..., :3] = srgb_eotf(p[..., :3])
        tex.decoded[level] = p
    return tex.decoded[level][y, x]


def _axis(u, n, filt):
    """float32 decisions of one axis: (i0, t) -- t is None for NEAREST."""
    f = F32(F32(u) * F32(n))
    if filt == NEAREST:
        return int(math.floor(float(f))), None
    f = F32(f - F32(0.5))
    fl = math.floor(float(f))
    return int(fl), float(F32(f - F32(fl)))


def sample_level(tex, uv, level, filt):
    h, w = tex.levels[level].shape[:2]
    ix, tx = _axis(uv[0], w, filt)
    iy, ty = _axis(uv[1], h, filt)
    if filt == NEAREST:
        return texel(tex, level, wrap(ix, w, tex.wrap_s), wrap(iy, h, tex.wrap_t))
    x0, x1, y0, y1 = wrap(ix, w, tex.wrap_s), wrap(ix + 1, w, tex.wrap_s), wrap(iy, h, tex.wrap_t), wrap(iy + 1, h, tex.wrap_t)
    a, b, c, d = texel(tex, level, x0, y0), texel(tex, level, x1, y0), texel(tex, level, x0, y1), texel(tex, level, x1, y1)
    return (a * (1 - tx) + b * tx) * (1 - ty) + (c * (1 - tx) + d * tx) * ty


def _nearest_uv_outcomes(tex, uv, level, filt, uv_band):
    """uvs standing for every texel choice a NEAREST fetch at `level` can make within uv_band of uv."""
    if filt != NEAREST or uv_band == 0.0:
        return [uv]
    h, w = tex.levels[level].shape[:2]
    us, vs = {float(uv[0])}, {float(uv[1])}
    for d in (-uv_band, uv_band):
        if math.floor((uv[0] + d) * w) != math.floor(uv[0] * w):
            us.add(float(uv[0] + d))
        if math.floor((uv[1] + d) * h) != math.floor(uv[1] * h):
            vs.add(float(uv[1] + d))
    return [(a, b) for a in sorted(us) for b in sorted(vs)]


class Outcome:
    """value: rgba float64; spread: the largest |b - a| over the pairs of adjacent level values a LINEAR level selection blends at, or next to,
    this level of detail (0 without level blend) -- times the error of the level of detail it bounds what that error does to the value."""

    def __init__(self, value, spread=0.0, what="", a=None, b=None):
        self.value, self._spread, self.what, self.a, self.b = value, float(spread), what, a, b  # a, b: the two level values actually blended, or None

    def spread(self):
        return self._spread


def sample(tex, uv, lod, lod_band=0.0, uv_band=0.0):
    """Every outcome of the fetch.  uv: float32 pair when uv_band == 0 (decisions restated exactly), float64 otherwise; lod: None (no
    gradient: level 0, magnification), or the level of detail before clamping -- exact when lod_band == 0."""
    last = len(tex.levels) - 1
    plans = []  # (tag, level0, level1 or None, f, filter)
    if lod is None:
        plans.append(("mag", 0, None, 0.0, tex.mag))
    else:
        if lod - lod_band <= 0.0:
            plans.append(("mag", 0, None, 0.0, tex.mag))
        if lod + lod_band > 0.0:
            lo = max(lod, 0.0)
            if tex.mip == NEAREST:
                for cand in sorted({lo - lod_band, lo, lo + lod_band}):
                    lv = min(int(math.floor(min(max(cand, 0.0), last) + 0.5)), last)
                    plans.append(("min", lv, None, 0.0, tex.min))
            else:
                lc = min(lo, float(last))
                l0 = min(int(math.floor(lc)), last)
                l1 = min(l0 + 1, last)
                f = lc - l0
                plans.append(("min", l0, l1 if (l1 != l0 and f > 0.0) else None, f, tex.min))
    if len(plans) > 1 and tex.mag == tex.min and tex.mip == LINEAR and plans[0][0] == "mag":
        plans = plans[1:]  # same filter on both sides of lod = 0 and a blend that starts at f = 0: continuous there (the spread term covers it), one outcome
    outs = []
    for tag, l0, l1, f, filt in plans:
        for p in _nearest_uv_outcomes(tex, uv, l0, filt, uv_band):
            a = sample_level(tex, p, l0, filt)
            if tag == "mag" or tex.mip == NEAREST:
                o = Outcome(a, what="%s L%d" % (tag, l0))
            else:
                # (the coarser level's NEAREST choice under a uv band: the finer level's representative uv stands for both; a coarser texel is wider)
                b = sample_level(tex, p, l1, filt) if l1 is not None else a
                spread = float(np.abs(b - a).max())
                if l0 > 0 and f < 0.5:  # the level of detail may fall just below l0: the pair below blends there
                    spread = max(spread, float(np.abs(sample_level(tex, p, l0 - 1, filt) - a).max()))
                if l1 is None and l0 < last:  # f == 0 exactly: the pair above, entered at any f > 0
                    spread = max(spread, float(np.abs(sample_level(tex, p, l0 + 1, filt) - a).max()))
                o = Outcome(a * (1 - f) + b * f, spread, "%s L%d+%.3f" % (tag, l0, f), a if l1 is not None else None, b if l1 is not None else None)
            if not any(np.array_equal(o.value, q.value) for q in outs):
                outs.append(o)
    return outs


def uv_conditioning(tex, uv, lod, lod_band, uv_band):
    """The change of the (first) reference outcome under uv +- uv_band: the bound's share for a coordinate known only to the band."""
    base = sample(tex, uv, lod, lod_band, 0.0)[0].value
    worst = 0.0
    for du, dv in ((uv_band, 0), (-uv_band, 0), (0, uv_band), (0, -uv_band)):
        worst = max(worst, float(np.abs(sample(tex, (uv[0] + du, uv[1] + dv), lod, lod_band, 0.0)[0].value - base).max()))
    return worst


# ---- texture coordinate and level of detail of a slot --------------------------------------------------------------------------------------------
def transform_uv(U, t):
    """KHR_texture_transform as packed in MiGltfTextureInfo.uvTransform (uv' = (u, v, 1) * M, M three rows of two).  Returns (uv, band): float32 and 0
    without rotation, float64 and UV_BAND with one."""
    U = [F32(x) for x in U]
    if U[1] == 0 and U[2] == 0:
        return (F32(F32(F32(t[0]) * U[0]) + U[4]), F32(F32(F32(t[1]) * U[3]) + U[5])), 0.0
    t0, t1 = float(F32(t[0])), float(F32(t[1]))
    return (t0 * float(U[0]) + t1 * float(U[2]) + float(U[4]), t0 * float(U[1]) + t1 * float(U[3]) + float(U[5])), UV_BAND


def lod_of(U, tex_grad, width, height):
    """Level of detail of an isotropic footprint of `tex_grad` (in the primitive's uv per pixel) after the transform: the gradient vectors are
    (tex_grad, 0) and (0, tex_grad) in uv, scaled to texels per axis; lod = log2 of the longer one (Vulkan 16.5.7, rho_max).  None when there is no
    gradient.  float64 from the float32 inputs."""
    g = float(F32(tex_grad))
    if not g > 0.0:
        return None
    U = [float(F32(x)) for x in U]
    rx = math.hypot(U[0] * g * width, U[1] * g * height)
    ry = math.hypot(U[2] * g * width, U[3] * g * height)
    rho = max(rx, ry)
    return math.log2(rho) if rho > 0.0 else -126.0


# ---- the material ---------------------------------------------------------------------------------------------------------------------------------
MIN_ROUGHNESS = float(F32(0.0014142))
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


class Tables:
    """What `material` reads of a scene: materials (MiGltfShadeMaterial), texture infos (MiGltfTextureInfo), texture records (Tex or None)."""

    def __init__(self, materials, infos, textures):
        self.materials, self.infos, self.textures = materials, infos, textures

    @classmethod
    def from_scene(cls, scene):
        d = scene.desc.contents
        return cls([d.materials[i] for i in range(d.numMaterials)], [d.textureInfos[i] for i in range(d.numTextureInfos)],
                   [tex_from_desc(d.textures[i]) for i in range(d.numTextures)])


def material(tables, material_id, tc0, tc1, tex_grad, vertex_colour=(1, 1, 1, 1), frame=((1, 0, 0), (0, 1, 0), (0, 0, 1)), lod_band=LOD_BAND,
             perturb=None, pick=0):
    """The PbrMaterial fields the debug views expose, float64.  tc0 / tc1: the hit's float32 texture coordinates; tex_grad: its float32 footprint
    (uv per pixel; 0: none).  Returns (fields, info): info["undecided"] is the number of slots with more than one outcome -- outcome `pick` is
    used, the last where a slot has fewer -- and info["outcomes"] the largest number at a slot; info["spread"][field] the largest |b - a| of the
    level blends behind a field (for the delta_lod term), info["cond"][field] the conditioning of the fetches under a rotated coordinate;
    info["taps"] the number of fetches.  perturb: rgba added to every fetched texel value (the bounds of the derived fields come from the change
    of this function under it)."""
    m = tables.materials[material_id]
    info = {"undecided": 0, "spread": {}, "cond": {}, "taps": 0, "outcomes": 1}
    cur = [None]

    def tex(slot):
        ti = tables.infos[slot]
        info["taps"] += 1
        if not (0 <= ti.index < len(tables.textures)) or tables.textures[ti.index] is None:
            return np.ones(4)
        t = tables.textures[ti.index]
        U = list(ti.uvTransform)
        uv, band = transform_uv(U, tc0 if ti.texCoord == 0 else tc1)
        lod = lod_of(U, tex_grad, t.width, t.height)
        outs = sample(t, uv, lod, lod_band if lod is not None else 0.0, band)
        if len(outs) > 1:
            info["undecided"] += 1
        for f in cur[0]:
            info["spread"][f] = max(info["spread"].get(f, 0.0), outs[min(pick, len(outs) - 1)].spread())
            if band:
                info["cond"][f] = max(info["cond"].get(f, 0.0), uv_conditioning(t, uv, lod, lod_band if lod is not None else 0.0, band))
        o = outs[min(pick, len(outs) - 1)]
        info["outcomes"] = max(info["outcomes"], len(outs))
        return o.value if perturb is None else o.value + perturb

    def T(slot, *fields):
        cur[0] = fields
        return tex(slot)

    p = {}
    vc = np.asarray(vertex_colour, np.float64)
    if m.pbrModel == 1:  # KHR_materials_pbrSpecularGlossiness, converted as gltf_material_eval.h.slang:136-161
        diffuse = np.array(m.pbrDiffuseFactor[:], np.float64) * vc
        gloss, spec = float(m.pbrGlossinessFactor), np.array(m.pbrSpecularFactor[:], np.float64)
        if m.pbrDiffuseTexture:
            diffuse = diffuse * T(m.pbrDiffuseTexture, "baseColor", "opacity", "metallic")
        if m.pbrSpecularGlossinessTexture:
            s = T(m.pbrSpecularGlossinessTexture, "baseColor", "metallic", "roughness")
            spec, gloss = spec * s[:3], gloss * s[3]
        x = min(max((spec.max() - 0.05) / 0.04, 0.0), 1.0)
        p["metallic"] = x * x * (3 - 2 * x)
        p["baseColor"] = spec if p["metallic"] > 0 else np.clip(diffuse[:3] / (1 - 0.04 * (1 - p["metallic"])), 0, 1)
        p["roughness"] = np.full(2, (1 - gloss) ** 2)
        p["opacity"] = diffuse[3]
    else:
        base = np.array(m.pbrBaseColorFactor[:], np.float64) * vc
        if m.pbrBaseColorTexture:
            base = base * T(m.pbrBaseColorTexture, "baseColor", "opacity")
        p["baseColor"], p["opacity"] = base[:3], base[3]
        rough, metal = float(m.pbrRoughnessFactor), float(m.pbrMetallicFactor)
        if m.pbrMetallicRoughnessTexture:
            s = T(m.pbrMetallicRoughnessTexture, "roughness", "metallic")
            rough, metal = rough * s[1], metal * s[2]  # glTF 3.9.2: roughness in G, metalness in B
        rough = max(rough, MIN_ROUGHNESS)
        p["roughness"] = np.full(2, rough * rough)
        p["metallic"] = min(max(metal, 0.0), 1.0)
    p["occlusion"] = float(m.occlusionStrength)
    if m.occlusionTexture:
        p["occlusion"] = 1 + float(m.occlusionStrength) * (T(m.occlusionTexture, "occlusion")[0] - 1)
    Tn, Bn, Nn = (np.asarray(v, np.float64) for v in frame)
    p["N"], p["T"], p["B"] = Nn, Tn, Bn
    update = False
    if m.normalTexture:
        c = T(m.normalTexture, "N", "T", "B", "Nc")[:3] * 2 - 1
        c = c * np.array([m.normalTextureScale, m.normalTextureScale, 1.0])
        p["N"] = _unit(Tn * c[0] + Bn * c[1] + Nn * c[2])
        update = True
    p["emissive"] = np.array(m.emissiveFactor[:], np.float64)
    if m.emissiveTexture:
        p["emissive"] = p["emissive"] * T(m.emissiveTexture, "emissive")[:3]
    p["emissive"] = np.maximum(p["emissive"], 0)
    p["specularColor"] = np.array(m.specularColorFactor[:], np.float64)
    if m.specularColorTexture:
        p["specularColor"] = p["specularColor"] * T(m.specularColorTexture, "specularColor")[:3]
    p["specular"] = float(m.specularFactor)
    if m.specularTexture:
        p["specular"] *= T(m.specularTexture, "specular")[3]
    p["transmission"] = float(m.transmissionFactor)
    if m.transmissionTexture:
        p["transmission"] *= T(m.transmissionTexture, "transmission", "opacity")[0]
    p["clearcoat"], p["clearcoatRoughness"], p["Nc"] = float(m.clearcoatFactor), float(m.clearcoatRoughness), p["N"]
    if m.clearcoatTexture:
        p["clearcoat"] *= T(m.clearcoatTexture, "clearcoat")[0]
    if m.clearcoatRoughnessTexture:
        p["clearcoatRoughness"] *= T(m.clearcoatRoughnessTexture, "clearcoatRoughness")[1]
    if m.clearcoatNormalTexture:
        c = T(m.clearcoatNormalTexture, "Nc")[:3] * 2 - 1
        p["Nc"] = _unit(p["T"] * c[0] + p["B"] * c[1] + p["Nc"] * c[2])
    p["clearcoatRoughness"] = max(p["clearcoatRoughness"], float(F32(0.001)))
    irid, thick = float(m.iridescenceFactor), float(m.iridescenceThicknessMaximum)
    if m.iridescenceTexture:
        irid *= T(m.iridescenceTexture, "iridescence")[0]
    if m.iridescenceThicknessTexture:
        g = T(m.iridescenceThicknessTexture, "iridescenceThickness", "iridescence")[1]
        thick = float(m.iridescenceThicknessMinimum) * (1 - g) + float(m.iridescenceThicknessMaximum) * g
    p["iridescence"], p["iridescenceThickness"] = (irid if thick > 0 else 0.0), thick
    strength = float(m.anisotropyStrength)
    if strength > 0:
        d = np.array([1.0, 0.0])
        if m.anisotropyTexture:
            a = T(m.anisotropyTexture, "roughness", "T", "B")
            d = _unit(a[:2] * 2 - 1)
            strength *= a[2]
        s2 = strength * strength
        p["roughness"] = np.array([p["roughness"][1] * (1 - s2) + s2, p["roughness"][1]])
        s, c = float(m.anisotropyRotation[0]), float(m.anisotropyRotation[1])
        d = np.array([c * d[0] + s * d[1], c * d[1] - s * d[0]])
        p["T"] = p["T"] * d[0] + p["B"] * d[1]
        update = True
    if update:
        b = _unit(np.cross(p["N"], p["T"]))
        sign = 1.0 if np.dot(Bn, b) >= 0 else -1.0
        p["B"] = b * sign
        p["T"] = _unit(np.cross(p["B"], p["N"]) * sign)
    p["sheenColor"] = np.array(m.sheenColorFactor[:], np.float64)
    if m.sheenColorTexture:
        p["sheenColor"] = p["sheenColor"] * T(m.sheenColorTexture, "sheenColor")[:3]
    p["sheenRoughness"] = float(m.sheenRoughnessFactor)
    if m.sheenRoughnessTexture:
        p["sheenRoughness"] *= T(m.sheenRoughnessTexture, "sheenRoughness")[3]
    p["sheenRoughness"] = max(p["sheenRoughness"], MIN_ROUGHNESS)
    p["diffuseTransmissionFactor"] = float(m.diffuseTransmissionFactor)
    if m.diffuseTransmissionTexture:
        p["diffuseTransmissionFactor"] *= T(m.diffuseTransmissionTexture, "diffuseTransmissionFactor")[3]
    p["diffuseTransmissionColor"] = np.array(m.diffuseTransmissionColor[:], np.float64)
    if m.diffuseTransmissionColorTexture:
        p["diffuseTransmissionColor"] = p["diffuseTransmissionColor"] * T(m.diffuseTransmissionColorTexture, "diffuseTransmissionColor")[:3]
    return p, info


# ---- the tables of the device, built by their rule (csrc/device/pt_scene.h) -------------------------------------------------------------------------
TEXREF_DTYPE = np.dtype([("uv", "<f4", (6,)), ("level0", "<u4"), ("width", "<u2"), ("height", "<u2"), ("numLevels", "u1"), ("srgb", "u1"), ("magFilter", "u1"),
                         ("minFilter", "u1"), ("mipmapMode", "u1"), ("wrapS", "u1"), ("wrapT", "u1"), ("texCoord", "u1"), ("pad", "<u4")])
CORETEX_DTYPE = np.dtype([("level0", "<u4"), ("wh", "<u4"), ("flags", "<u4"), ("ref", "<u4")])
assert TEXREF_DTYPE.itemsize == 44 and CORETEX_DTYPE.itemsize == 16
CT_FAST, CT_SRGB, CT_TEXCOORD1, CT_TRANSFORM, CT_MIP_LINEAR, CT_WRAPS_SHIFT, CT_WRAPT_SHIFT, CT_LEVELS_SHIFT = 1, 2, 4, 8, 16, 8, 10, 16


def device_tables(tables):
    """Texel pool, footprint records (the rule of k_texture_quads: the four texels (x, y), (x+1, y), (x, y+1), (x+1, y+1) of every texel, the
    neighbour clamped under CLAMP_TO_EDGE and wrapped to 0 otherwise), DevTexRef per texture info, DevCoreTex per material and core slot
    (deriveTextureRecords), and the 256-entry sRGB table in float32 arithmetic."""
    pool, quads, level0 = [], [], []
    off = 0
    for t in tables.textures:
        level0.append(off)
        for lv in t.levels:
            h, w = lv.shape[:2]
            px = lv.reshape(h, w, 4).astype(np.uint32)
            words = px[..., 0] | (px[..., 1] << 8) | (px[..., 2] << 16) | (px[..., 3] << 24)
            x1 = np.minimum(np.arange(w) + 1, w - 1) if t.wrap_s == CLAMP else (np.arange(w) + 1) % w
            y1 = np.minimum(np.arange(h) + 1, h - 1) if t.wrap_t == CLAMP else (np.arange(h) + 1) % h
            q = np.stack([words, words[:, x1], words[y1, :], words[y1][:, x1]], -1)
            pool.append(words.reshape(-1))
            quads.append(q.reshape(-1, 4))
            off += h * w
    pool = np.ascontiguousarray(np.concatenate(pool), np.uint32)
    quads = np.ascontiguousarray(np.concatenate(quads), np.uint32)
    refs = np.zeros(max(len(tables.infos), 1), TEXREF_DTYPE)
    for i, ti in enumerate(tables.infos):
        refs[i]["uv"] = list(ti.uvTransform)
        refs[i]["texCoord"] = ti.texCoord
        if 0 <= ti.index < len(tables.textures):
            t = tables.textures[ti.index]
            for k, v in (("level0", level0[ti.index]), ("width", t.width), ("height", t.height), ("numLevels", len(t.levels)), ("srgb", t.srgb), ("magFilter", t.mag),
                         ("minFilter", t.min), ("mipmapMode", t.mip), ("wrapS", t.wrap_s), ("wrapT", t.wrap_t)):
                refs[i][k] = v
    core = np.zeros(max(len(tables.materials), 1) * 5, CORETEX_DTYPE)
    for mi, m in enumerate(tables.materials):
        for k, slot in enumerate((m.pbrBaseColorTexture, m.normalTexture, m.pbrMetallicRoughnessTexture, m.emissiveTexture, m.occlusionTexture)):
            c = core[mi * 5 + k]
            c["ref"] = slot
            if slot == 0 or slot >= len(tables.infos):
                continue
            r = refs[slot]
            c["level0"], c["wh"] = r["level0"], int(r["width"]) | (int(r["height"]) << 16)
            fast = r["width"] > 0 and r["magFilter"] == LINEAR and r["minFilter"] == LINEAR and r["wrapS"] != MIRROR and r["wrapT"] != MIRROR
            c["flags"] = (CT_FAST if fast else 0) | (CT_SRGB if r["srgb"] else 0) | (CT_TEXCOORD1 if r["texCoord"] else 0) \
                | (0 if r["uv"].tobytes() == np.array(IDENTITY, "<f4").tobytes() else CT_TRANSFORM) | (CT_MIP_LINEAR if r["mipmapMode"] == LINEAR else 0) \
                | (int(r["wrapS"]) << CT_WRAPS_SHIFT) | (int(r["wrapT"]) << CT_WRAPT_SHIFT) | (int(r["numLevels"]) << CT_LEVELS_SHIFT)
    c = np.arange(256, dtype=np.float32) / F32(255.0)
    lut = np.where(c <= F32(0.04045), c / F32(12.92), np.power((c + F32(0.055)) / F32(1.055), F32(2.4))).astype(np.float32)
    return pool, quads, refs, core, lut
