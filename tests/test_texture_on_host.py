"""CPU tier of the texel-level texture tests: the texture fetch (getTextureRef), the core-slot path (coreTexPlan -> coreTexIssue -> coreTexFinish) and
evaluateMaterial<false, false> / <false, true> of csrc/device/pt_shading.h, compiled for the host through tests/host_shim/texture_on_host.cpp with
plain IEEE arithmetic (g++ -ffp-contract=off), against the float64 reference of tests/texture_ref.py on the cases of tests/texture_cases.py.  The tables
the shim reads -- texel pool, footprint records (the rule of k_texture_quads), DevTexRef, DevCoreTex, the sRGB table -- are built in numpy from the
host loader's scene (texture_ref.device_tables).  No GPU needed.

Bounds (texture_ref): a fetch without a level blend FETCH_BOUND = 20 u (u = 2^-24: 14 u the float32 sRGB table entry against the float64 curve, 6 u the
pinned bilinear blend) = 1.19e-6; a trilinear one 3 u more plus |b - a| * DELTA_LOD_LIBM (8.2e-7 levels: derived there from the float32 chain and
libm's log2f, not measured); under a rotated coordinate the reference's own change under uv +- UV_BAND on top.  A material field: the change of the
reference under the fetch bound added to every texel value with every sign pattern (its own conditioning -- no free constant), plus 8 u of the field's
magnitude for its own handful of roundings (factor, vertex colour, square, lerp, normalisation).  The undecided share (texture_ref: more than one
outcome within the bands) must be 0 in the classes with lod <= 0 and no rotation -- the shim's arithmetic is the restated float32 arithmetic -- and at
most 2 % elsewhere.  Each test prints per class the case count, the worst difference as a share of its bound, and the undecided share."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import texture_cases as tc
import texture_ref as tr
from texture_ref import F32, FETCH_BOUND, TRILINEAR_EXTRA, U
from vk_gltf_renderer_amd import pathtracer as ptmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("baseColor", 3), ("opacity", 1), ("roughness", 2), ("metallic", 1), ("emissive", 3), ("occlusion", 1), ("N", 3), ("T", 3), ("B", 3), \
    ("Ng", 3), ("specular", 1), ("specularColor", 3), ("transmission", 1), ("clearcoat", 1), ("clearcoatRoughness", 1), ("Nc", 3), ("iridescence", 1), \
    ("iridescenceThickness", 1), ("sheenColor", 3), ("sheenRoughness", 1), ("diffuseTransmissionFactor", 1), ("diffuseTransmissionColor", 3)
CP_FAST, CP_TWO, CP_SLOW = 1, 2, 128
MAX_UNDECIDED = 0.02
# the lattice of the power-of-two sizes as designed (texture_cases.lattice_uv: 2 n + 5 values per axis and eight fixed points per combination; 54 such
# combinations): coordinates EXACTLY on a decision boundary of their filter (a texel edge under NEAREST, a texel centre under LINEAR), and exactly on a seam
MIN_ON_BOUNDARY, MIN_ON_SEAM = 600, 250


class ShimTexTables(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("quads", C.c_void_p), ("refs", C.c_void_p), ("lut", C.c_void_p)]


@pytest.fixture(scope="module")
def shim(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("texture_shim") / "libtexture_on_host.so")
    d = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-I" + d, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"), "-o", out, os.path.join(d, "texture_on_host.cpp")], check=True)
    L = C.CDLL(out)
    VP, I = C.c_void_p, C.c_int
    L.dev_get_texture.argtypes = [VP, I, VP, VP, VP, VP]
    L.dev_core_texture.argtypes = [VP, I, VP, VP, VP, VP, VP, VP]
    L.dev_evaluate_material.argtypes = [VP, VP, VP, I, VP, VP]
    L.dev_evaluate_material.restype = I
    sizes = (I * 4)()
    L.dev_tex_sizes(sizes)
    from vk_gltf_renderer_amd import _capi as capi
    assert list(sizes) == [tr.TEXREF_DTYPE.itemsize, tr.CORETEX_DTYPE.itemsize, C.sizeof(capi.MiGltfShadeMaterial), C.sizeof(capi.MiGltfTextureInfo)]
    offs = (I * len(FIELDS))()
    L.n_floats = L.dev_tex_material_layout(offs)
    L.offsets = {name: (int(o), n) for (name, n), o in zip(FIELDS, offs)}
    return L


class World:
    """A loaded scene, its reference tables and its device tables."""

    def __init__(self, path):
        self.scene = ptmod.Scene(path)
        self.tables = tr.Tables.from_scene(self.scene)
        self.pool, self.quads, self.refs, self.core, self.lut = tr.device_tables(self.tables)

    def ctx(self, quads=True):
        t = ShimTexTables(self.pool.ctypes.data, self.quads.ctypes.data if quads else None, self.refs.ctypes.data, self.lut.ctypes.data)
        return t

    def fetch(self, L, slots, tcs, grads, quads=True):
        slots, tcs, grads = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(tcs, np.float32), np.ascontiguousarray(grads, np.float32)
        out = np.zeros((len(slots), 4), np.float32)
        t = self.ctx(quads)
        L.dev_get_texture(C.addressof(t), len(slots), slots.ctypes.data, tcs.ctypes.data, grads.ctypes.data, out.ctypes.data)
        return out

    def core_fetch(self, L, cores, slots, tcs, grads, quads=True):
        slots, tcs, grads = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(tcs, np.float32), np.ascontiguousarray(grads, np.float32)
        words = np.ascontiguousarray(self.core[np.asarray(cores)]).view(np.uint32).reshape(-1, 4)
        out, path = np.zeros((len(slots), 4), np.float32), np.zeros(len(slots), np.uint32)
        t = self.ctx(quads)
        L.dev_core_texture(C.addressof(t), len(slots), words.ctypes.data, slots.ctypes.data, tcs.ctypes.data, grads.ctypes.data, out.ctypes.data, path.ctypes.data)
        return out, path

    def tex_of(self, slot):
        return self.tables.textures[self.tables.infos[slot].index]


@pytest.fixture(scope="module")
def zoo(built, tmp_path_factory):
    path, combos = tc.build_sampler_zoo(str(tmp_path_factory.mktemp("texture_zoo") / "sampler_zoo.glb"))
    w = World(path)
    w.combos = combos
    for c in combos:  # the loader's records are the designed ones
        for slot in (w.tables.materials[c.index].emissiveTexture, w.tables.materials[c.index].occlusionTexture):
            t = w.tex_of(slot)
            assert (t.width, t.height, len(t.levels), t.mag, t.min, t.mip, t.wrap_s, t.wrap_t) == (*c.size, c.levels, c.mag, c.min, c.mip, c.wrap_s, c.wrap_t), c
        assert w.tex_of(w.tables.materials[c.index].emissiveTexture).srgb and not w.tex_of(w.tables.materials[c.index].occlusionTexture).srgb
    return w


@pytest.fixture(scope="module")
def matzoo(built, tmp_path_factory):
    path, entries = tc.build_material_zoo(str(tmp_path_factory.mktemp("texture_matzoo") / "material_zoo.glb"))
    w = World(path)
    w.entries = entries
    return w


class Tally:
    def __init__(self):
        self.rows = {}

    def add(self, cls, diff, bound, outcomes):
        r = self.rows.setdefault(cls, [0, 0.0, 0, None])
        r[0] += 1
        if diff / bound > r[1]:
            r[1] = diff / bound
        r[2] += 1 if outcomes > 1 else 0

    def report(self, title, zero_classes=()):
        shown = {}
        for cls, (n, worst, und, _) in self.rows.items():  # (many classes: printed per first part of the name)
            g = shown.setdefault(cls if len(self.rows) <= 60 else cls.split("/")[0], [0, 0.0, 0])
            g[0], g[1], g[2] = g[0] + n, max(g[1], worst), g[2] + und
        for cls in sorted(shown):
            n, worst, und = shown[cls]
            print("TEXMEASURE %s/%-28s n %6d  worst %.3f of its bound  undecided %.4f" % (title, cls, n, worst, und / n))
        for cls, (n, worst, und, _) in self.rows.items():
            assert worst <= 1.0, (title, cls, worst)
            assert und / n <= MAX_UNDECIDED, (title, cls, und / n)
            if cls in zero_classes or any(cls.startswith(z) for z in zero_classes):
                assert und == 0, (title, cls, und)


def _match(got, outs, bound_of):
    """Smallest diff / bound over the outcomes, as (diff, bound)."""
    best = None
    for o in outs:
        d, b = float(np.abs(got.astype(np.float64) - o.value).max()), bound_of(o)
        if best is None or d / b < best[0] / best[1]:
            best = (d, b)
    return best


def test_tables_follow_the_device_rules(zoo):
    """The footprint record of a texel holds it and its right / lower / diagonal neighbours under the wrap modes, whatever the level size."""
    w = zoo
    off = 0
    for t in w.tables.textures:
        for lv in t.levels:
            h, wd = lv.shape[:2]
            words = w.pool[off:off + h * wd].reshape(h, wd)
            q = w.quads[off:off + h * wd].reshape(h, wd, 4)
            for y, x in itertools.product(range(h), range(wd)):
                x1 = min(x + 1, wd - 1) if t.wrap_s == tr.CLAMP else (x + 1) % wd
                y1 = min(y + 1, h - 1) if t.wrap_t == tr.CLAMP else (y + 1) % h
                assert tuple(q[y, x]) == (words[y, x], words[y, x1], words[y1, x], words[y1, x1])
            off += h * wd
    assert off == len(w.pool)
    # the table against the float64 curve: within the 14 u the value bound grants it
    assert np.abs(w.lut.astype(np.float64) - tr.srgb_eotf(np.arange(256) / 255.0)).max() <= 14 * U


def test_loader_packs_the_texture_transform_of_the_specification(matzoo):
    """KHR_texture_transform: uv' = T R S uv with R = [[cos, sin], [-sin, cos]].  Under a uniform scale the reference renderer's packing
    (src/tinygltf_utils.hpp:67-78, whose rotation and scale commute only then) is the specification's; the cases keep to it."""
    idx = {e["name"]: i for i, e in enumerate(matzoo.entries)}
    for name, (off, rot, sc) in (("transform_offset", ((0.375, -1.25), 0.0, (1.0, 1.0))), ("transform_scale", ((0.1, 0.2), 0.0, (2.0, 0.5))),
                                 ("transform_rotation_uv1", ((0.25, -0.5), 0.3, (1.5, 1.5)))):
        ti = matzoo.tables.infos[matzoo.tables.materials[idx[name]].emissiveTexture]
        c, s = np.cos(rot), np.sin(rot)
        M = np.array([[1, 0, off[0]], [0, 1, off[1]], [0, 0, 1]]) @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]]) @ np.diag([sc[0], sc[1], 1.0])
        for uv in ((0.3, 0.7), (-1.5, 2.25)):
            want = M @ np.array([uv[0], uv[1], 1.0])
            got, _ = tr.transform_uv(list(ti.uvTransform), uv)
            assert abs(float(got[0]) - want[0]) < 1e-6 and abs(float(got[1]) - want[1]) < 1e-6, (name, uv)
        assert ti.texCoord == (1 if "uv1" in name else 0)


def test_level0_classes(shim, zoo):
    """No gradient (pixelAngle = 0): level 0 through the magnification filter.  Lattice, CLAMP_TO_EDGE footprints and random uv over [-3.5, 5.5]^2, every
    size, every pair of wrap modes, both filters, the sRGB and the linear twin, with footprint records and without."""
    cases = tc.level0_cases(zoo.combos)
    tally, same = Tally(), []
    on_boundary = on_seam = 0
    for twin in ("colour", "data"):
        slots = [getattr(zoo.tables.materials[c.index], "emissiveTexture" if twin == "colour" else "occlusionTexture") for c, _, _ in cases]
        tcs = np.array([[uv[0], uv[1], 9.0, 9.0] for _, uv, _ in cases], np.float32)
        got = zoo.fetch(shim, slots, tcs, np.zeros(len(cases)))
        got4 = zoo.fetch(shim, slots, tcs, np.zeros(len(cases)), quads=False)
        for k, (c, uv, cls) in enumerate(cases):
            outs = tr.sample(zoo.tex_of(slots[k]), (tcs[k, 0], tcs[k, 1]), None)
            for tag, g in (("", got), ("/four-gathers", got4)):
                d, b = _match(g[k], outs, lambda o: FETCH_BOUND)
                tally.add("%s/%s/%s%s" % (cls, c.kind, twin, tag), d, b, len(outs))
            if twin == "colour" and cls == "lattice" and c.pot:
                fu, fv = float(tcs[k, 0]) * c.size[0], float(tcs[k, 1]) * c.size[1]
                shift = 0.0 if c.kind == "NN" else 0.5
                on_boundary += int((fu - shift) == np.floor(fu - shift) or (fv - shift) == np.floor(fv - shift))
                on_seam += int(float(tcs[k, 0]) in (0.0, 1.0) or float(tcs[k, 1]) in (0.0, 1.0))
        same.append(got.tobytes() == got4.tobytes())
    print("TEXMEASURE level0 lattice (power-of-two sizes): exactly on a decision boundary %d, exactly on a seam %d" % (on_boundary, on_seam))
    assert on_boundary >= MIN_ON_BOUNDARY and on_seam >= MIN_ON_SEAM
    tally.report("level0", zero_classes=("lattice", "clamp", "random"))
    assert all(same)  # footprint records == four gathers, bit for bit


def _lod_inputs(zoo, cases, twin):
    slots = [getattr(zoo.tables.materials[c.index], "emissiveTexture" if twin == "colour" else "occlusionTexture") for c, _, _ in cases]
    tcs = np.array([[uv[0], uv[1], 9.0, 9.0] for _, uv, _ in cases], np.float32)
    grads = np.array([tc.tex_grad_of(tc.height_of(c, lod)) for c, _, lod in cases], np.float32)
    return slots, tcs, grads


def test_lod_classes(shim, zoo):
    """Level selection: lod < 0, 0, between and on every level, the last level and beyond, NEAREST and LINEAR selection, the mixed filter pairs."""
    cases = tc.lod_cases(zoo.combos)
    tally, same = Tally(), []
    for twin in ("colour", "data"):
        slots, tcs, grads = _lod_inputs(zoo, cases, twin)
        got = zoo.fetch(shim, slots, tcs, grads)
        same.append(got.tobytes() == zoo.fetch(shim, slots, tcs, grads, quads=False).tobytes())
        for k, (c, uv, lod) in enumerate(cases):
            t = zoo.tex_of(slots[k])
            lod64 = tr.lod_of(tr.IDENTITY, grads[k], t.width, t.height)
            assert abs(lod64 - lod) < 1e-6  # the case is the designed one
            outs = tr.sample(t, (tcs[k, 0], tcs[k, 1]), lod64, tr.LOD_BAND)
            d, b = _match(got[k], outs, lambda o: FETCH_BOUND + TRILINEAR_EXTRA + o.spread() * tr.DELTA_LOD_LIBM)
            cls = "lod<=0" if lod <= 0 else ("nearest-mip" if c.mip == tr.NEAREST else "linear-mip")
            tally.add("%s/%s/%s" % (cls, c.kind, twin), d, b, len(outs))
    tally.report("lod", zero_classes=("lod<=0",))
    assert all(same)  # footprint records == four gathers, bit for bit


def _transform_cases(matzoo, seed=8, n=200):
    rng = np.random.default_rng(seed)
    out = []
    for i, e in enumerate(matzoo.entries):
        if not e["name"].startswith("transform_"):
            continue
        slot = matzoo.tables.materials[i].emissiveTexture
        for k in range(n):
            tc0, tc1 = rng.uniform(-3.5, 5.5, 2), rng.uniform(-2.0, 3.0, 2)
            lod = (None, 1.25, 0.75)[k % 3]
            out.append((e["name"], slot, np.array([*tc0, *tc1], np.float32), lod))
    return out


def test_transform_classes(shim, matzoo):
    """KHR_texture_transform: offset, scale (exactly restated), rotation over TEXCOORD_1 (float64 coordinate with its band)."""
    cases = _transform_cases(matzoo)
    tally = Tally()
    slots = [s for _, s, _, _ in cases]
    tcs = np.stack([t for _, _, t, _ in cases])
    grads = []
    for name, slot, t4, lod in cases:
        info, t = matzoo.tables.infos[slot], matzoo.tex_of(slot)
        if lod is None:
            grads.append(0.0)
        else:  # the footprint that gives this lod under the transform's scale
            unit = tr.lod_of(list(info.uvTransform), 1.0, t.width, t.height)
            grads.append(2.0 ** (lod - unit))
    grads = np.array(grads, np.float32)
    got = matzoo.fetch(shim, slots, tcs, grads)
    same = got.tobytes() == matzoo.fetch(shim, slots, tcs, grads, quads=False).tobytes()
    for k, (name, slot, t4, lod) in enumerate(cases):
        info, t = matzoo.tables.infos[slot], matzoo.tex_of(slot)
        Um = list(info.uvTransform)
        uv, band = tr.transform_uv(Um, t4[0:2] if info.texCoord == 0 else t4[2:4])
        assert (band > 0) == ("rotation" in name)
        lod64 = tr.lod_of(Um, grads[k], t.width, t.height)
        lb = tr.LOD_BAND if lod64 is not None else 0.0
        outs = tr.sample(t, uv, lod64, lb, band)
        cond = tr.uv_conditioning(t, uv, lod64, lb, band) if band else 0.0
        d, b = _match(got[k], outs, lambda o: FETCH_BOUND + TRILINEAR_EXTRA + o.spread() * tr.DELTA_LOD_LIBM + cond)
        tally.add("%s/%s" % (name, "lod<=0" if lod is None else "lod>0"), d, b, len(outs))
    tally.report("transform", zero_classes=("transform_offset/lod<=0", "transform_scale/lod<=0"))
    assert same  # footprint records == four gathers, bit for bit


def test_core_path_is_the_general_fetch_bit_for_bit(shim, zoo, matzoo):
    """coreTexPlan -> coreTexIssue -> coreTexFinish through the DevCoreTex record of a slot == getTextureRef, with footprint records and without
    (TexCtx::quads == nullptr), on every case of the classes above; the fast path, its two-level shape and the fall-back all occur."""
    seen = {CP_FAST: 0, CP_TWO: 0, CP_SLOW: 0}
    l0, ld = tc.level0_cases(zoo.combos), tc.lod_cases(zoo.combos)
    for core_k, field in ((0, "pbrBaseColorTexture"), (4, "occlusionTexture"), (3, "emissiveTexture"), (2, "pbrMetallicRoughnessTexture")):
        cases = [(c, uv, None) for c, uv, _ in l0] + ld
        slots = [getattr(zoo.tables.materials[c.index], field) for c, _, _ in cases]
        cores = [5 * c.index + core_k for c, _, _ in cases]
        tcs = np.array([[uv[0], uv[1], 9.0, 9.0] for _, uv, _ in cases], np.float32)
        grads = np.array([0.0 if lod is None else tc.tex_grad_of(tc.height_of(c, lod)) for c, _, lod in cases], np.float32)
        want = zoo.fetch(shim, slots, tcs, grads)
        for quads in (True, False):
            got, path = zoo.core_fetch(shim, cores, slots, tcs, grads, quads)
            assert got.tobytes() == want.tobytes(), (field, quads, int((got != want).any(1).sum()))
            if quads:
                for bit in seen:
                    seen[bit] += int(((path & bit) != 0).sum())
                fast = np.array([c.kind == "LL" and tr.MIRROR not in (c.wrap_s, c.wrap_t) for c, _, _ in cases])
                assert (((path & CP_FAST) != 0) == fast).all() and (((path & CP_SLOW) != 0) == ~fast).all()
            else:
                assert ((path & CP_SLOW) != 0).all()
    # the transformed slots (CT_TRANSFORM, CT_TEXCOORD1) of the material zoo
    tcases = _transform_cases(matzoo)
    idx = {e["name"]: i for i, e in enumerate(matzoo.entries)}
    slots, cores = [s for _, s, _, _ in tcases], [5 * idx[name] + 3 for name, _, _, _ in tcases]
    tcs = np.stack([t for _, _, t, _ in tcases])
    grads = np.array([0.0 if lod is None else 2.0 ** lod / 16 for _, _, _, lod in tcases], np.float32)
    want = matzoo.fetch(shim, slots, tcs, grads)
    for quads in (True, False):
        got, path = matzoo.core_fetch(shim, cores, slots, tcs, grads, quads)
        assert got.tobytes() == want.tobytes(), ("transform", quads)
        assert (matzoo.core[cores]["flags"] & tr.CT_TRANSFORM).all()
    print("TEXMEASURE core path: fast %d, of them two-level %d, general %d" % (seen[CP_FAST], seen[CP_TWO], seen[CP_SLOW]))
    assert seen[CP_FAST] > 5000 and seen[CP_TWO] > 500 and seen[CP_SLOW] > 5000


SIGNS = [np.array([a, b, c, a], np.float64) for a in (1, -1) for b in (1, -1) for c in (1, -1)]


def field_bounds(tables, mat, tc0, tc1, grad, vc, frame, delta_lod):
    """(fields, bounds, info) of the reference: per field the largest change under the fetch bound added to every texel value with every sign
    pattern, plus 8 u of the field's magnitude."""
    p, info = tr.material(tables, mat, tc0, tc1, grad, vc, frame)
    e = FETCH_BOUND + TRILINEAR_EXTRA + max(info["spread"].values(), default=0.0) * delta_lod + max(info["cond"].values(), default=0.0)
    bounds = {k: 0.0 for k in p}
    for s in SIGNS:
        q, _ = tr.material(tables, mat, tc0, tc1, grad, vc, frame, perturb=s * e)
        for k in p:
            bounds[k] = max(bounds[k], float(np.abs(np.asarray(q[k], np.float64) - p[k]).max()))
    for k in p:
        bounds[k] += 8 * U * max(1.0, float(np.abs(p[k]).max()))
    return p, bounds, info


@pytest.mark.parametrize("core", [0, 1])
def test_material_fields(shim, matzoo, core):
    """evaluateMaterial<false, CORE>: every map slot on its own, all together, the specular-glossiness model, a slot without a valid texture, vertex
    colour; channel assignments per the specifications (texture_ref.material).  Level 0 and a trilinear footprint; two shading frames."""
    tally = Tally()
    taps_seen = 0
    c30, s30 = np.cos(0.5), np.sin(0.5)
    frames = (((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((c30, 0, -s30), (0, 1, 0), (s30, 0, c30)))
    t = matzoo.ctx(True)
    for n, (i, uv) in enumerate(tc.material_cases(matzoo.entries)):
        e = matzoo.entries[i]
        tc0 = np.array(uv, np.float32)
        tc1 = np.array([4.0 - float(tc0[1]) / 2, float(tc0[0]) / 2], np.float32)
        grad = F32(0.0 if n % 2 else 2.0 ** 1.25 / 16)
        vc = np.array(e["vertex_colour"], np.float32)
        frame = frames[n % 3 == 0]
        want, bounds, info = field_bounds(matzoo.tables, i, tc0, tc1, grad, vc.astype(np.float64), frame, tr.DELTA_LOD_LIBM)
        inp = np.array([*tc0, *tc1, grad, *vc, *frame[0], *frame[1], *frame[2]], np.float32)
        out = np.zeros(shim.n_floats, np.float32)
        core5 = np.ascontiguousarray(matzoo.core[5 * i:5 * i + 5]).view(np.uint32)
        m = matzoo.tables.materials[i]
        taps = shim.dev_evaluate_material(C.addressof(t), C.addressof(m), core5.ctypes.data, core, inp.ctypes.data, out.ctypes.data)
        assert taps == info["taps"], (e["name"], taps, info["taps"])
        taps_seen = max(taps_seen, taps)
        for name, ref in want.items():
            o, k = shim.offsets[name]
            d = float(np.abs(out[o:o + k].astype(np.float64) - ref).max())
            tally.add("%s/%s" % (e["name"], name), d, bounds[name], 1 + info["undecided"])
    assert taps_seen == 18  # the material with every map: 5 core slots and 13 of the extensions
    tally.report("material core=%d" % core)
