"""The scenes and cases shared by the two tiers of the texel-level texture tests (tests/test_texture_on_host.py, tests/test_gpu_texture_views.py):
the smallest shapes at which the fetch (csrc/device/pt_shading.h) can go wrong.  No GPU needed.

Geometry.  Every combination of texture and sampler, and every material of the zoo, gets a unit quad of its own in z = 0, on its own render node at
(2 col, 2 row, 0); uv0 = -4 + 16 (x, y) over the quad (texel density 16 uv per world unit), uv1 = (4 - v0 / 2, u0 / 2) (swapped and mirrored: a u / v
mix-up cannot pass).  Corners, uvs and the lattice ray origins of the power-of-two textures are dyadic with few bits, so barycentrics and uv
interpolation are exact there -- which the GPU tier proves through MI_VIZ_TEXCOORD0/1 instead of assuming it.

Textures.  Random 8-bit RGBA, four independent channels; the bytes 0, 255 and the two sides of the sRGB knee (10, 11) forced in.  Sizes: 1x1, 2x2, 8x2
(the height reaches 1 two levels before the width), 16x16 (five levels), 5x3 and 7x7 (no powers of two: the general modulo, mip sizes that floor).  Each
combination has a colour twin (sRGB: emissive and base colour read it) and a data twin with other bytes (linear: occlusion and metallic-roughness).

Level of detail.  Under NEAREST level selection k + 0.5 IS the decision boundary, a coin toss for any float32 evaluation: the nearest-selection
samplers get k, k + 0.25 and k + 0.75 instead (k + 0.75 is what tells floor(lod + 0.5) from floor(lod)); lod = 0 exactly goes to the samplers whose
magnification and minification filters agree (there both sides of the boundary are one outcome), the mixed ones get -0.25 and 0.25.
"""
import math

import numpy as np

import texture_ref as tr
from texture_ref import CLAMP, F32, LINEAR, MIRROR, NEAREST, REPEAT

SIZES = ((1, 1), (2, 2), (8, 2), (16, 16), (5, 3), (7, 7))  # (width, height)
GL_WRAP = {REPEAT: 10497, CLAMP: 33071, MIRROR: 33648}
# sampler kinds: glTF (magFilter, minFilter) -> the record's (mag, min, mip); the loader's mipmapMode follows magFilter
FILTERS = {"LL": (9729, 9987), "NN": (9728, 9984), "LN": (9729, 9986), "NL": (9728, 9985)}
FILTER_RECORD = {"LL": (LINEAR, LINEAR, LINEAR), "NN": (NEAREST, NEAREST, NEAREST), "LN": (LINEAR, NEAREST, LINEAR), "NL": (NEAREST, LINEAR, NEAREST)}
UV_LO, UV_SPAN = -4.0, 16.0
DENSITY = 16.0             # uv per world unit
PIXEL_ANGLE = 2.0 ** -12   # texGrad = PIXEL_ANGLE * height * DENSITY
RANDOM_LO, RANDOM_HI = -3.5, 5.5


def image(rng, w, h):
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    forced = np.array([[10, 11, 255, 0], [0, 255, 11, 10], [255, 0, 10, 11], [11, 10, 0, 255]], np.uint8)
    flat = img.reshape(-1, 4)
    for k in range(min(len(flat), 4)):
        flat[(k * 5) % len(flat)] = forced[k]
    return img


def quad():
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    uv0 = (UV_LO + UV_SPAN * pos[:, :2]).astype(np.float32)
    uv1 = np.stack([4.0 - uv0[:, 1] / 2, uv0[:, 0] / 2], 1).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    tng = np.tile(np.array([1, 0, 0, 1], np.float32), (4, 1))
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    return pos, idx, nrm, uv0, uv1, tng


def node_origin(i):
    return 2.0 * (i % 16), 2.0 * (i // 16)


def ray_xy(i, uv):
    """World (x, y) in float32 of the ray that meets quad i at uv0 = uv."""
    ox, oy = node_origin(i)
    return F32(ox + (float(uv[0]) - UV_LO) / UV_SPAN), F32(oy + (float(uv[1]) - UV_LO) / UV_SPAN)


def expected_uv(i, x, y, scale=(1.0, 1.0)):
    """float64 uv0 and uv1 of the hit of a -z ray through float32 (x, y) on quad i (affine)."""
    ox, oy = node_origin(i)
    u, v = UV_LO + UV_SPAN * (float(x) - ox) / scale[0], UV_LO + UV_SPAN * (float(y) - oy) / scale[1]
    return (u, v), (4.0 - v / 2, u / 2)


# ---- the sampler zoo --------------------------------------------------------------------------------------------------------------------------------
class Combo:
    def __init__(self, index, size, wrap_s, wrap_t, kind):
        self.index, self.size, self.wrap_s, self.wrap_t, self.kind = index, size, wrap_s, wrap_t, kind
        self.mag, self.min, self.mip = FILTER_RECORD[kind]
        self.levels = 1 + int(math.floor(math.log2(max(size))))
        self.pot = all((n & (n - 1)) == 0 for n in size)

    def __repr__(self):
        return "%dx%d %s%s %s" % (self.size[0], self.size[1], "RCM"[self.wrap_s], "RCM"[self.wrap_t], self.kind)


def sampler_zoo_combos():
    out = []
    for size in SIZES:
        for ws in (REPEAT, CLAMP, MIRROR):
            for wt in (REPEAT, CLAMP, MIRROR):
                for kind in ("LL", "NN"):
                    out.append(Combo(len(out), size, ws, wt, kind))
    for size in ((16, 16), (8, 2), (7, 7), (5, 3)):
        for w in (REPEAT, CLAMP, MIRROR):
            for kind in ("LN", "NL"):
                out.append(Combo(len(out), size, w, w, kind))
    return out


def build_sampler_zoo(path, seed=11):
    """One material per combination: emissive and base colour read the colour twin, occlusion and metallic-roughness the data twin."""
    from vk_gltf_renderer_amd import scenegen
    rng = np.random.default_rng(seed)
    b = scenegen.GlbBuilder()
    combos = sampler_zoo_combos()
    images = {size: (b.image(image(rng, *size)), b.image(image(rng, *size))) for size in SIZES}
    pos, idx, nrm, uv0, uv1, tng = quad()
    for c in combos:
        smp = b.sampler(mag=FILTERS[c.kind][0], min_=FILTERS[c.kind][1], wrap_s=GL_WRAP[c.wrap_s], wrap_t=GL_WRAP[c.wrap_t])
        colour, data = b.texture(images[c.size][0], smp), b.texture(images[c.size][1], smp)
        m = b.material({"pbrMetallicRoughness": {"baseColorTexture": {"index": colour}, "metallicRoughnessTexture": {"index": data}},
                        "emissiveTexture": {"index": colour}, "emissiveFactor": [1.0, 1.0, 1.0], "occlusionTexture": {"index": data}})
        ox, oy = node_origin(c.index)
        b.node(mesh=b.mesh([b.primitive(pos, idx, nrm, uv0, uv1=uv1, tangents=tng, material=m)]), translation=[ox, oy, 0.0])
    b.camera_node((16.0, 8.0, 40.0), (16.0, 8.0, 0.0))
    return b.save(path), combos


def lattice_axis(n):
    """Texel centres and edges from one texel outside 0 to one outside 1, half a texel inside and outside the seams included: k / (2 n)."""
    return [k / (2.0 * n) for k in range(-2, 2 * n + 3)]


def lattice_uv(w, h):
    U, V = lattice_axis(w), lattice_axis(h)
    pts = [(U[i % len(U)], V[(3 * i + 1) % len(V)]) for i in range(max(len(U), len(V)))]
    pts += [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (-0.5 / w, -0.5 / h), (1.0 + 0.5 / w, 0.5 / h), (0.5, 0.0), (1.0, 0.5)]
    return pts


def clamp_uv(w, h):
    """First texel of the bilinear footprint ix < 0, ix = -1 exactly, ix = w - 1 and ix >= w (what CLAMP_TO_EDGE duplicates), per axis."""
    fx = (-1.8, -0.5, w - 0.2, w + 1.2)
    fy = (h + 1.2, h - 0.2, -0.5, -1.8)
    return [(a / w, b / h) for a, b in zip(fx, fy)] + [(-0.5 / w, 0.3), (0.3, -0.5 / h)]


def random_uv(rng, n, dyadic_bits=12):
    """Over [-3.5, 5.5]^2: beyond one period either side for REPEAT and beyond two for MIRRORED_REPEAT at the small sizes.  On a 2^-bits grid of the quad, so
    that the ray origins are exact."""
    s = rng.integers(int((RANDOM_LO - UV_LO) / UV_SPAN * 2 ** dyadic_bits), int((RANDOM_HI - UV_LO) / UV_SPAN * 2 ** dyadic_bits), (n, 2))
    return [(UV_LO + UV_SPAN * a / 2.0 ** dyadic_bits, UV_LO + UV_SPAN * b / 2.0 ** dyadic_bits) for a, b in s]


def level0_cases(combos, seed=5, n_random=24):
    """(combo, uv, class) of the magnification class: no gradient (pixelAngle = 0)."""
    rng = np.random.default_rng(seed)
    out = []
    for c in combos:
        if c.kind not in ("LL", "NN"):
            continue
        w, h = c.size
        for uv in lattice_uv(w, h):
            out.append((c, uv, "lattice"))
        for uv in clamp_uv(w, h):
            out.append((c, uv, "clamp"))
        for uv in random_uv(rng, n_random):
            out.append((c, uv, "random"))
    return out


def lods_of(c):
    last = c.levels - 1
    same = c.mag == c.min
    lods = [-1.0] + ([0.0] if same else [-0.25, 0.25]) + [0.5 if c.mip == LINEAR else 0.25]
    for k in range(1, last + 1):
        lods += [float(k), k + 0.5] if c.mip == LINEAR else [float(k), k + 0.25, k + 0.75]
    if c.mip == NEAREST:
        lods.append(0.75)
    lods.append(last + 1.5)  # beyond the last level
    return lods


def lod_cases(combos, seed=6, n_uv=4):
    """(combo, uv, lod) of the minification classes: wraps RR, CC, MM and RC, every filter kind, every size."""
    rng = np.random.default_rng(seed)
    out = []
    for c in combos:
        if (c.wrap_s, c.wrap_t) not in ((REPEAT, REPEAT), (CLAMP, CLAMP), (MIRROR, MIRROR), (REPEAT, CLAMP)):
            continue
        for lod in lods_of(c):
            for uv in random_uv(rng, n_uv):
                out.append((c, uv, lod))
    return out


def height_of(c, lod):
    """Ray origin height at which the ray cone gives combination c the level of detail lod: rho = PIXEL_ANGLE * h * DENSITY * max(W, H)."""
    return 2.0 ** lod / (PIXEL_ANGLE * DENSITY * max(c.size))


def tex_grad_of(height, scale=1.0):
    return PIXEL_ANGLE * height * DENSITY * scale


# ---- the material zoo -------------------------------------------------------------------------------------------------------------------------------
def _ext(name, **kw):
    return {"extensions": {name: kw}}


def build_material_zoo(path, subset="all", seed=12):
    """Every map slot on its own, one material with all of them, the specular-glossiness model, a slot without a valid texture, the texture
    transforms, a non-uniformly scaled node; subset "core": the core slots only (no extension lobes: the scene-wide SIMPLE kernels run).
    Returns (path, entries): entries[i] = dict(name, node scale)."""
    from vk_gltf_renderer_amd import scenegen
    rng = np.random.default_rng(seed)
    b = scenegen.GlbBuilder()
    lin, nst = b.sampler(), b.sampler(mag=9728, min_=9984)
    mir = b.sampler(wrap_s=GL_WRAP[MIRROR], wrap_t=GL_WRAP[MIRROR])

    def tex(size=(16, 16), smp=lin):
        return {"index": b.texture(b.image(image(rng, *size)), smp)}

    def nmap():  # a normal-map-like image: z well above zero, so that the perturbed normal stays well conditioned
        img = image(rng, 16, 16)
        img[..., 2] = 128 + img[..., 2] // 2
        return {"index": b.texture(b.image(img), lin)}

    def mr(**kw):
        d = {"pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.8, 0.7, 1.0], "metallicFactor": 0.75, "roughnessFactor": 0.9}}
        for k, v in kw.items():
            if k == "pbr":
                d["pbrMetallicRoughness"].update(v)
            elif k == "extensions":
                d.setdefault("extensions", {}).update(v)
            else:
                d[k] = v
        return d
    rot = {"KHR_texture_transform": {"offset": [0.25, -0.5], "rotation": 0.3, "scale": [1.5, 1.5], "texCoord": 1}}
    core = [
        ("base_colour_vertex_colour", mr(pbr={"baseColorTexture": tex()})),
        ("metallic_roughness", mr(pbr={"metallicRoughnessTexture": tex()})),
        ("occlusion", mr(occlusionTexture=dict(tex(), strength=0.7))),
        ("emissive", mr(emissiveTexture=tex(), emissiveFactor=[0.5, 2.0, 1.0])),
        ("normal", mr(normalTexture=dict(nmap(), scale=0.8))),
        ("invalid_texture", mr(pbr={"baseColorTexture": {"index": 4000}}, emissiveTexture={"index": 4001}, emissiveFactor=[0.25, 0.5, 0.75])),
        ("transform_offset", mr(emissiveTexture=dict(tex(), extensions={"KHR_texture_transform": {"offset": [0.375, -1.25]}}), emissiveFactor=[1.0, 1.0, 1.0])),
        ("transform_scale", mr(emissiveTexture=dict(tex((7, 7), mir), extensions={"KHR_texture_transform": {"scale": [2.0, 0.5], "offset": [0.1, 0.2]}}),
                               emissiveFactor=[1.0, 1.0, 1.0])),
        ("transform_rotation_uv1", mr(emissiveTexture=dict(tex(), texCoord=1, extensions=rot), emissiveFactor=[1.0, 1.0, 1.0])),
        ("transform_rotation_nearest", mr(emissiveTexture=dict(tex((7, 7), nst), texCoord=1, extensions=rot), emissiveFactor=[1.0, 1.0, 1.0])),
        ("scaled_node", mr(emissiveTexture=tex(), emissiveFactor=[1.0, 1.0, 1.0])),
        ("core_together", mr(pbr={"baseColorTexture": tex(), "metallicRoughnessTexture": tex()}, occlusionTexture=dict(tex(), strength=0.5), emissiveTexture=tex(),
                             emissiveFactor=[1.0, 0.5, 0.25], normalTexture=nmap())),
    ]
    everything = {"KHR_materials_clearcoat": {"clearcoatFactor": 0.9, "clearcoatTexture": tex(), "clearcoatRoughnessFactor": 0.8, "clearcoatRoughnessTexture": tex(),
                                              "clearcoatNormalTexture": nmap()},
                  "KHR_materials_sheen": {"sheenColorFactor": [0.9, 0.6, 0.3], "sheenColorTexture": tex(), "sheenRoughnessFactor": 0.7, "sheenRoughnessTexture": tex()},
                  "KHR_materials_specular": {"specularFactor": 0.8, "specularTexture": tex(), "specularColorFactor": [0.7, 0.8, 0.9], "specularColorTexture": tex()},
                  "KHR_materials_transmission": {"transmissionFactor": 0.6, "transmissionTexture": tex()},
                  "KHR_materials_iridescence": {"iridescenceFactor": 0.9, "iridescenceTexture": tex(), "iridescenceThicknessMinimum": 150.0,
                                                "iridescenceThicknessMaximum": 900.0, "iridescenceThicknessTexture": tex()},
                  "KHR_materials_anisotropy": {"anisotropyStrength": 0.8, "anisotropyRotation": 0.6, "anisotropyTexture": tex()},
                  "KHR_materials_diffuse_transmission": {"diffuseTransmissionFactor": 0.7, "diffuseTransmissionTexture": tex(),
                                                         "diffuseTransmissionColorFactor": [0.5, 0.6, 0.9], "diffuseTransmissionColorTexture": tex()}}
    ext = [
        ("clearcoat", mr(**_ext("KHR_materials_clearcoat", clearcoatFactor=0.9, clearcoatTexture=tex()))),
        ("clearcoat_roughness", mr(**_ext("KHR_materials_clearcoat", clearcoatFactor=1.0, clearcoatRoughnessFactor=0.8, clearcoatRoughnessTexture=tex()))),
        ("clearcoat_normal", mr(**_ext("KHR_materials_clearcoat", clearcoatFactor=1.0, clearcoatNormalTexture=nmap()))),
        ("sheen_colour", mr(**_ext("KHR_materials_sheen", sheenColorFactor=[0.9, 0.6, 0.3], sheenColorTexture=tex()))),
        ("sheen_roughness", mr(**_ext("KHR_materials_sheen", sheenColorFactor=[1.0, 1.0, 1.0], sheenRoughnessFactor=0.7, sheenRoughnessTexture=tex()))),
        ("specular", mr(**_ext("KHR_materials_specular", specularFactor=0.8, specularTexture=tex()))),
        ("specular_colour", mr(**_ext("KHR_materials_specular", specularColorFactor=[0.7, 0.8, 0.9], specularColorTexture=tex()))),
        ("transmission", mr(**_ext("KHR_materials_transmission", transmissionFactor=0.6, transmissionTexture=tex()))),
        ("iridescence", mr(**_ext("KHR_materials_iridescence", iridescenceFactor=0.9, iridescenceTexture=tex()))),
        ("iridescence_thickness", mr(**_ext("KHR_materials_iridescence", iridescenceFactor=1.0, iridescenceThicknessMinimum=150.0, iridescenceThicknessMaximum=900.0,
                                            iridescenceThicknessTexture=tex()))),
        ("anisotropy", mr(**_ext("KHR_materials_anisotropy", anisotropyStrength=0.8, anisotropyRotation=0.6, anisotropyTexture=tex()))),
        ("diffuse_transmission", mr(**_ext("KHR_materials_diffuse_transmission", diffuseTransmissionFactor=0.7, diffuseTransmissionTexture=tex()))),
        ("diffuse_transmission_colour", mr(**_ext("KHR_materials_diffuse_transmission", diffuseTransmissionFactor=1.0, diffuseTransmissionColorFactor=[0.5, 0.6, 0.9],
                                                  diffuseTransmissionColorTexture=tex()))),
        ("specular_glossiness", {"extensions": {"KHR_materials_pbrSpecularGlossiness": {"diffuseFactor": [0.9, 0.8, 0.7, 1.0], "diffuseTexture": tex(),
                                                                                      "specularFactor": [0.9, 0.9, 0.9], "glossinessFactor": 0.8,
                                                                                      "specularGlossinessTexture": tex()}}}),
        ("all_together", mr(pbr={"baseColorTexture": tex(), "metallicRoughnessTexture": tex()}, occlusionTexture=dict(tex(), strength=0.5), emissiveTexture=tex(),
                            emissiveFactor=[1.0, 0.5, 0.25], normalTexture=nmap(), extensions=everything)),
    ]
    pos, idx, nrm, uv0, uv1, tng = quad()
    entries = []
    for i, (name, mat) in enumerate(core + (ext if subset == "all" else [])):
        m = b.material(mat)
        colours = np.tile(np.array([200, 100, 50, 255], np.uint8), (4, 1)) if name == "base_colour_vertex_colour" else None
        scale = [2.0, 1.0, 1.0] if name == "scaled_node" else [1.0, 1.0, 1.0]
        ox, oy = node_origin(i)
        b.node(mesh=b.mesh([b.primitive(pos, idx, nrm, uv0, uv1=uv1, colors=colours, tangents=tng, material=m)]), translation=[ox, oy, 0.0], scale=scale)
        entries.append({"name": name, "scale": (scale[0], scale[1]), "vertex_colour": (200 / 255.0, 100 / 255.0, 50 / 255.0, 1.0) if colours is not None else (1, 1, 1, 1)})
    b.camera_node((16.0, 8.0, 40.0), (16.0, 8.0, 0.0))
    return b.save(path), entries


def material_cases(entries, seed=7, n_uv=10):
    """(entry index, uv0) per material: random points and four lattice points of a 16-texel axis."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(len(entries)):
        for uv in random_uv(rng, n_uv) + [(0.0, 0.0), (1.0, 0.5 / 16), (1.5 / 16, 1.0), (-0.5 / 16, 2.0)]:
            out.append((i, uv))
    return out


# ---- the debug views in float64 (shaders/common.h.slang:32-164 of the reference renderer; MiVisualization) ---------------------------------------------
def view_colour(mode, p):
    """(rgb float64 BEFORE the OETF, through_oetf) of debug view `mode` (its MI_VIZ_* name) for material fields p."""
    s3 = lambda x: np.full(3, float(x))  # noqa: E731
    r = p["roughness"]
    table = {
        "BASE_COLOR": (lambda: p["baseColor"], True), "METALLIC": (lambda: s3(p["metallic"]), True), "ROUGHNESS": (lambda: np.array([r[0], r[1], r[0]]), True),
        "NORMAL_SHADING": (lambda: p["N"] * 0.5 + 0.5, True), "TANGENT": (lambda: p["T"] * 0.5 + 0.5, False), "BITANGENT": (lambda: p["B"] * 0.5 + 0.5, False),
        "EMISSIVE": (lambda: p["emissive"], False), "OPACITY": (lambda: s3(p["opacity"] * (1 - p["transmission"])), False),
        "OCCLUSION": (lambda: s3(p["occlusion"]), False), "CLEARCOAT_FACTOR": (lambda: s3(p["clearcoat"]), False),
        "CLEARCOAT_ROUGHNESS": (lambda: s3(p["clearcoatRoughness"]), False), "CLEARCOAT_NORMAL": (lambda: p["Nc"] * 0.5 + 0.5, False),
        "SHEEN_COLOR": (lambda: p["sheenColor"], False), "SHEEN_ROUGHNESS": (lambda: s3(p["sheenRoughness"]), False),
        "SPECULAR_FACTOR": (lambda: s3(p["specular"]), False), "SPECULAR_COLOR": (lambda: p["specularColor"], False),
        "TRANSMISSION_FACTOR": (lambda: s3(p["transmission"]), False), "IRIDESCENCE_FACTOR": (lambda: s3(p["iridescence"]), False),
        "IRIDESCENCE_THICKNESS": (lambda: s3(p["iridescenceThickness"] / 1200.0), False),
        "ANISOTROPY_STRENGTH": (lambda: s3(math.sqrt(min(max((r[0] - r[1]) / max(1 - r[1], 1e-5), 0.0), 1.0))), False),
        "DIFFUSE_TRANSMISSION_FACTOR": (lambda: s3(p["diffuseTransmissionFactor"]), False),
        "DIFFUSE_TRANSMISSION_COLOR": (lambda: p["diffuseTransmissionColor"], False),
        "GUIDE_ALBEDO": (lambda: p["baseColor"], False), "GUIDE_NORMAL": (lambda: p["N"], False),  # the denoiser guides of a RENDERED frame
    }
    fn, oetf = table[mode]
    return np.asarray(fn(), np.float64), oetf


SIGNS8 = [np.array([a, b, c, a], np.float64) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
SIGNS2 = [np.ones(4), -np.ones(4)]


def mixes_channels(m):
    """Whether a field of this material depends on several channels of one texel (normal maps, the anisotropy direction, the specular-glossiness
    conversion): then every sign pattern of the perturbation is tried, else the two uniform ones (each component follows one channel)."""
    return bool(m.normalTexture or m.clearcoatNormalTexture or m.anisotropyTexture or m.pbrModel == 1)


def reference_views(tables, mat, tc0, tc1, grad, vc, frame, delta_lod, views, pick=0):
    """{view: (colour, bound)} of the reference and the info of texture_ref.material.  The bound of a view before the OETF: the largest change of the
    reference under the fetch bound (FETCH_BOUND, the level blend's 3 u and |b - a| * delta_lod, the conditioning under a rotated coordinate) added to
    every texel value, over the sign patterns -- the reference's own conditioning, which is what bounds normals and tangents -- plus 8 u of the
    view's magnitude for the handful of roundings of the field itself.  Through the OETF: that times its largest slope 12.92, plus OETF_ABS."""
    p, info = tr.material(tables, mat, tc0, tc1, grad, vc, frame, pick=pick)
    e = tr.FETCH_BOUND + tr.TRILINEAR_EXTRA + max(info["spread"].values(), default=0.0) * delta_lod + max(info["cond"].values(), default=0.0)
    lin = {v: view_colour(v, p) for v in views}
    bound = {v: 0.0 for v in views}
    if info["taps"]:
        for s in (SIGNS8 if mixes_channels(tables.materials[mat]) else SIGNS2):
            q, _ = tr.material(tables, mat, tc0, tc1, grad, vc, frame, perturb=s * e, pick=pick)
            for v in views:
                bound[v] = max(bound[v], float(np.abs(view_colour(v, q)[0] - lin[v][0]).max()))
    out = {}
    for v in views:
        c, oetf = lin[v]
        b = bound[v] + 8 * tr.U * max(1.0, float(np.abs(c).max()))
        out[v] = (tr.srgb_oetf(c), b * tr.OETF_SLOPE + tr.OETF_ABS) if oetf else (c, b)
    return out, info, p


VIEWS_CORE = ("BASE_COLOR", "METALLIC", "ROUGHNESS", "NORMAL_SHADING", "TANGENT", "BITANGENT", "EMISSIVE", "OPACITY", "OCCLUSION", "SPECULAR_FACTOR", "SPECULAR_COLOR")
VIEWS_EXT = ("CLEARCOAT_FACTOR", "CLEARCOAT_ROUGHNESS", "CLEARCOAT_NORMAL", "SHEEN_COLOR", "SHEEN_ROUGHNESS", "TRANSMISSION_FACTOR", "IRIDESCENCE_FACTOR",
             "IRIDESCENCE_THICKNESS", "ANISOTROPY_STRENGTH", "DIFFUSE_TRANSMISSION_FACTOR", "DIFFUSE_TRANSMISSION_COLOR")
