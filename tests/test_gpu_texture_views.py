"""GPU tier of the texel-level texture tests: the texture fetch, the DevTexRef / footprint tables and evaluateMaterial as the SHIPPED kernels run
them, asked texel by texel through the public API -- no device code of the tests, no library but the product's.

How.  Axis-aligned unit quads in z = 0, one per sampler / material, each on its own render node (tests/texture_cases.py); one exact ray per case
straight down -z from (x, y, h), bound with mi_pt_set_camera_rays (no jitter).  MI_VIZ_TEXCOORD0/1 return the device's own float32 uv of the hit:
the integer part is recovered from the affine float64 expectation (ambiguity above 1e-4 fails), the lattice of the power-of-two textures must equal
the intended float32 uv bit for bit, and every other case feeds the DEVICE's uv into the float64 reference (tests/texture_ref.py) -- an error of
the hit position can neither hide a sampler error nor pass for one.  The fields of PbrMaterial are read through the debug views (k_shade_viz) and
through the albedo / normal guides of an ordinary RENDERED frame (the default shade kernel).  h sets the ray-cone footprint, and so the level of
detail: rho = pixelAngle * h * texel density * max(W, H).

Bounds (texture_cases.reference_views, texture_ref): a raw view is bounded by the change of the reference under the fetch bound added to every texel
value (FETCH_BOUND = 20 u = 1.19e-6: the float32 sRGB table entry and the pinned bilinear blend; 3 u more and |b - a| * delta_lod for a level
blend), plus 8 u of the view's magnitude; a view through toSrgb by that times 12.92 plus srgbOetf's recorded error.  delta_lod, the error of the
device's level of detail in levels, is MEASURED below as max |device - reference| / |b - a| over the trilinear cases with |b - a| >= 0.05 (per
channel), printed on every run, and asserted at twice the recorded figure, never above 1e-4.  Undecided cases (more than one outcome within
texture_ref's bands) must match one outcome; their share is at most 2 % per class and 0 where lod <= 0 without rotation."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as pu
import texture_cases as tc
import texture_ref as tr
from texture_ref import F32
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod
from vk_gltf_renderer_amd._capi import Visualization as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = 64                      # at most 64 x 64 rays per frame
FLT_MAX = np.finfo(np.float32).max
# max |device - reference| / |b - a| over the trilinear class with |b - a| >= 0.05 (578 channel values), measured on an MI355X (printed as TEXMEASURE
# delta_lod by test_level_of_detail_classes); the assertion uses twice this, capped at the ceiling.  The figure is the whole difference over |b - a|,
# so it contains the decode and blend error of the two taps (about 1e-7 over 0.05) as well: the device's level of detail itself is better than this.
MEASURED = {"delta_lod": 1.979e-06}
DELTA_LOD_CEILING = 1e-4
MAX_UNDECIDED = 0.02
MIN_ON_BOUNDARY, MIN_ON_SEAM = 600, 250  # of the lattice class (tests/test_texture_on_host.py: as designed, 1386 and 648)


def delta_lod_bound():
    return min(2.0 * MEASURED["delta_lod"], DELTA_LOD_CEILING)


class Rig:
    """One tracer per scene; views are switched with set_frame_info, one frame of one sample per view."""

    def __init__(self, path):
        self.st = pu.Setup(path, SIDE, SIDE, max_depth=2)
        self.tr = ptmod.PathTracer(self.st.scene)
        self.tr.resize(SIDE, SIDE)
        self.tr.set_sky(self.st.sky)
        self.tables = tr.Tables.from_scene(self.st.scene)

    def close(self):
        self.tr.close()

    def render(self, rays, view, pixel_angle, guides=False):
        """rays: (n <= SIDE^2, 8).  The view's colour per ray (n, 3); with guides=True (albedo, normal) of a RENDERED frame instead."""
        n = len(rays)
        full = np.zeros((SIDE * SIDE, 8), np.float32)
        full[:] = [-64.0, -64.0, 1.0, 0.0, 0.0, 0.0, -1.0, FLT_MAX]  # the rest of the frame misses the scene
        full[:n] = rays
        self.tr.set_camera_rays(full.reshape(1, SIDE, SIDE, 8), unit=True)
        fi = self.st.frame_info
        fi.visualization = int(V.RENDERED if guides else V[view])
        self.tr.set_frame_info(fi)
        p = self.st.frame_params(0, 0)
        p.pixelAngle = float(pixel_angle)
        p.flags = capi.MI_PT_FIRST_FRAME | (capi.MI_PT_USE_OPTIX_DENOISER if guides else 0)
        self.tr.render_frame(p)
        if guides:
            a, nrm = self.tr.read_guides()
            return a.reshape(-1, 4)[:n, :3].copy(), nrm.reshape(-1, 4)[:n, :3].copy()
        return self.tr.read_accum().reshape(-1, 4)[:n, :3].copy()

    def selection(self, n):
        return self.tr.read_selection().reshape(-1)[:n].copy()


def make_rays(xyh):
    r = np.zeros((len(xyh), 8), np.float32)
    r[:, 0:3] = np.asarray(xyh, np.float32)
    r[:, 6], r[:, 7] = -1.0, FLT_MAX
    return r


def recover_uv(fract, expected):
    """The device's float32 uv from the TEXCOORD view (fract(uv), exact in float32 for these magnitudes) and the affine float64 expectation."""
    assert (fract[:, 2] == 0.0).all()
    fr = fract[:, :2]
    k = np.round(expected - fr.astype(np.float64))
    ambiguity = float(np.abs(expected - fr - k).max())
    assert ambiguity <= 1e-4, ambiguity
    return (k.astype(np.float32) + fr).astype(np.float32)


def device_uvs(rig, rays, nodes, exp0, exp1, pixel_angle):
    uv0 = recover_uv(rig.render(rays, "TEXCOORD0", pixel_angle), np.asarray(exp0, np.float64))
    sel = rig.selection(len(rays))
    assert (sel == np.asarray(nodes) + 1).all(), "a ray met another quad than its own"
    uv1 = recover_uv(rig.render(rays, "TEXCOORD1", pixel_angle), np.asarray(exp1, np.float64))
    return uv0, uv1


class Tally:
    def __init__(self):
        self.rows = {}

    def add(self, cls, ratio, outcomes, detail=None):
        r = self.rows.setdefault(cls, [0, 0.0, 0, None])
        if ratio > r[1]:
            r[3] = detail
        r[0], r[1], r[2] = r[0] + 1, max(r[1], ratio), r[2] + (1 if outcomes > 1 else 0)

    def report(self, title, zero_classes=()):
        shown = {}
        for cls, (n, worst, und, _) in self.rows.items():  # (many classes: printed per first part of the name)
            g = shown.setdefault(cls if len(self.rows) <= 30 else cls.split("/")[0], [0, 0.0, 0])
            g[0], g[1], g[2] = g[0] + n, max(g[1], worst), g[2] + und
        for cls in sorted(shown):
            n, worst, und = shown[cls]
            print("TEXMEASURE %s/%-30s n %5d  worst %.3f of its bound  undecided %.4f" % (title, cls, n, worst, und / n))
        for cls, (n, worst, und, detail) in self.rows.items():
            assert worst <= 1.0, (title, cls, worst, detail)
            assert und / n <= MAX_UNDECIDED, (title, cls, und / n)
            if any(cls.startswith(z) for z in zero_classes):
                assert und == 0, (title, cls, und)


def check(tables, cases, got, views, delta_lod, tally):
    """cases[k]: dict(mat, uv0, uv1, grad, vc, cls); got[view]: (n, 3).  Every view of a case must lie within its bound of ONE outcome of the reference."""
    frame = ((1, 0, 0), (0, 1, 0), (0, 0, 1))  # the quads' tangent frame (checked through TANGENT / BITANGENT / the normal guide on the unmapped materials)
    for k, c in enumerate(cases):
        best, outcomes, pick = None, 1, 0
        while pick < outcomes:
            ref, info, _ = tc.reference_views(tables, c["mat"], c["uv0"], c["uv1"], c["grad"], c["vc"], frame, delta_lod, views, pick)
            outcomes = info["outcomes"]
            ratio, worst_view = max((float(np.abs(got[v][k].astype(np.float64) - ref[v][0]).max()) / ref[v][1], v) for v in views)
            if best is None or ratio < best[0]:
                best = (ratio, worst_view)
            pick += 1
        tally.add(c["cls"], best[0], outcomes, (k, best[1], c["mat"], tuple(float(x) for x in c["uv0"]), float(c["grad"])))


def render_views(rig, rays, views, pixel_angle):
    got = {}
    for v in views:
        if v.startswith("GUIDE_"):
            if "GUIDE_ALBEDO" not in got:
                got["GUIDE_ALBEDO"], got["GUIDE_NORMAL"] = rig.render(rays, None, pixel_angle, guides=True)
        else:
            got[v] = rig.render(rays, v, pixel_angle)
    return got


def batches(n):
    return [slice(i, min(i + SIDE * SIDE, n)) for i in range(0, n, SIDE * SIDE)]


# ---- the sampler zoo ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zoo(built, tmp_path_factory):
    path, combos = tc.build_sampler_zoo(str(tmp_path_factory.mktemp("gpu_texture_zoo") / "sampler_zoo.glb"))
    rig = Rig(path)
    rig.path, rig.combos = path, combos
    yield rig
    rig.close()


ZOO_VIEWS = ("EMISSIVE", "OPACITY", "OCCLUSION", "BASE_COLOR", "METALLIC", "ROUGHNESS", "GUIDE_ALBEDO")


def _level0(combos):
    cases = tc.level0_cases(combos, n_random=12)
    xyh = [(*tc.ray_xy(c.index, uv), 1.0) for c, uv, _ in cases]
    return cases, make_rays(xyh)


def _lod(combos):
    cases = tc.lod_cases(combos, n_uv=2)
    xyh = [(*tc.ray_xy(c.index, uv), tc.height_of(c, lod)) for c, uv, lod in cases]
    return cases, make_rays(xyh)


def _zoo_uvs(rig, cases, rays, sl, pixel_angle):
    exp = [tc.expected_uv(c.index, rays[i, 0], rays[i, 1]) for i, (c, _, _) in zip(range(sl.start, sl.stop), cases[sl])]
    return device_uvs(rig, rays[sl], [c.index for c, _, _ in cases[sl]], [e[0] for e in exp], [e[1] for e in exp], pixel_angle)


def test_level0_classes_and_the_uv_proof(zoo):
    """pixelAngle = 0: no gradient, level 0 through the magnification filter.  Every size, every pair of wrap modes, both filters; the sRGB twin through
    EMISSIVE (raw), BASE_COLOR (toSrgb), the albedo guide (default kernel) and OPACITY (alpha), the linear twin through OCCLUSION (R), ROUGHNESS (G) and
    METALLIC (B)."""
    cases, rays = _level0(zoo.combos)
    tally = Tally()
    on_boundary = on_seam = exact = 0
    for sl in batches(len(cases)):
        uv0, uv1 = _zoo_uvs(zoo, cases, rays, sl, 0.0)
        for i, (c, uv, cls) in enumerate(cases[sl]):
            if cls == "lattice" and c.pot:  # dyadic all the way: the device's uv IS the intended one
                assert uv0[i, 0] == F32(uv[0]) and uv0[i, 1] == F32(uv[1]), (c, uv, uv0[i])
                exact += 1
                fu, fv = float(uv0[i, 0]) * c.size[0], float(uv0[i, 1]) * c.size[1]
                shift = 0.0 if c.kind == "NN" else 0.5
                on_boundary += int((fu - shift) == np.floor(fu - shift) or (fv - shift) == np.floor(fv - shift))
                on_seam += int(float(uv0[i, 0]) in (0.0, 1.0) or float(uv0[i, 1]) in (0.0, 1.0))
        got = render_views(zoo, rays[sl], ZOO_VIEWS, 0.0)
        todo = [dict(mat=c.index, uv0=uv0[i], uv1=uv1[i], grad=0.0, vc=(1, 1, 1, 1), cls="%s/%s" % (cls, c.kind)) for i, (c, uv, cls) in enumerate(cases[sl])]
        check(zoo.tables, todo, got, ZOO_VIEWS, 0.0, tally)
    print("TEXMEASURE level0 lattice: bit-exact uv %d, exactly on a decision boundary %d, exactly on a seam %d" % (exact, on_boundary, on_seam))
    assert on_boundary >= MIN_ON_BOUNDARY and on_seam >= MIN_ON_SEAM
    tally.report("level0", zero_classes=("lattice", "clamp", "random"))


LOD_VIEWS = ("EMISSIVE", "OCCLUSION", "OPACITY", "BASE_COLOR", "GUIDE_ALBEDO")


def test_level_of_detail_classes(zoo):
    """The level of detail per ray through the height of its origin: below 0, 0, between and on every level, the last level, beyond it; NEAREST and
    LINEAR level selection, the mixed filter pairs.  Measures delta_lod."""
    cases, rays = _lod(zoo.combos)
    tally = Tally()
    measured, n_measured = 0.0, 0
    for sl in batches(len(cases)):
        uv0, uv1 = _zoo_uvs(zoo, cases, rays, sl, tc.PIXEL_ANGLE)
        got = render_views(zoo, rays[sl], LOD_VIEWS, tc.PIXEL_ANGLE)
        todo = []
        for i, (c, uv, lod) in enumerate(cases[sl]):
            grad = tc.tex_grad_of(float(rays[sl][i, 2]))
            cls = "lod<=0" if lod <= 0 else ("nearest-mip" if c.mip == tr.NEAREST else "linear-mip")
            todo.append(dict(mat=c.index, uv0=uv0[i], uv1=uv1[i], grad=grad, vc=(1, 1, 1, 1), cls="%s/%s" % (cls, c.kind)))
            if cls == "linear-mip":  # the measurement: raw views of the two twins, per channel, where the two levels differ by 0.05 or more
                m = zoo.tables.materials[c.index]
                for slot, view, chans in ((m.emissiveTexture, "EMISSIVE", (0, 1, 2)), (m.occlusionTexture, "OCCLUSION", (0,))):
                    t = zoo.tables.textures[zoo.tables.infos[slot].index]
                    o = tr.sample(t, uv0[i], tr.lod_of(tr.IDENTITY, grad, t.width, t.height), tr.LOD_BAND)[0]
                    if o.a is None:
                        continue
                    for ch in chans:
                        if abs(o.b[ch] - o.a[ch]) >= 0.05:
                            measured = max(measured, abs(float(got[view][i, ch]) - o.value[ch]) / abs(o.b[ch] - o.a[ch]))
                            n_measured += 1
        check(zoo.tables, todo, got, LOD_VIEWS, delta_lod_bound(), tally)
    print("TEXMEASURE delta_lod  n %d  max |device - reference| / |b - a| = %.3e levels  (recorded %.3e, asserted %.3e)"
          % (n_measured, measured, MEASURED["delta_lod"], delta_lod_bound()))
    assert n_measured > 500
    assert measured <= delta_lod_bound()
    tally.report("lod", zero_classes=("lod<=0",))


def test_four_gather_path_in_a_child_process(zoo, tmp_path):
    """MI_PT_DIAG_NO_QUADS=1 (four texel gathers per bilinear tap, TexCtx::quads == nullptr) in a fresh process: the magnification class against the
    reference, and both classes bit for bit against this process's footprint-record path."""
    views = ("EMISSIVE", "OCCLUSION")
    (c0, r0), (c1, r1) = _level0(zoo.combos), _lod(zoo.combos)
    out = {}
    for name, rays, angle in (("level0", r0, 0.0), ("lod", r1, tc.PIXEL_ANGLE)):
        pad = np.zeros((len(batches(len(rays))), SIDE * SIDE, 8), np.float32)
        pad[:] = [-64.0, -64.0, 1.0, 0.0, 0.0, 0.0, -1.0, FLT_MAX]
        for b, sl in enumerate(batches(len(rays))):
            pad[b, :sl.stop - sl.start] = rays[sl]
        rp, op = str(tmp_path / (name + "_rays.npy")), str(tmp_path / (name + "_out.npy"))
        np.save(rp, pad)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "texture_views_child.py"), zoo.path, rp, repr(angle), ",".join(views), op],
                           env=dict(os.environ, MI_PT_DIAG_NO_QUADS="1"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        child = np.load(op)
        for b, sl in enumerate(batches(len(rays))):
            for k, v in enumerate(views):
                mine = zoo.render(rays[sl], v, angle)
                assert mine.tobytes() == child[b, k, :sl.stop - sl.start].tobytes(), (name, b, v)
        out[name] = child
    tally = Tally()
    for b, sl in enumerate(batches(len(c0))):
        uv0, uv1 = _zoo_uvs(zoo, c0, r0, sl, 0.0)
        got = {v: out["level0"][b, k, :sl.stop - sl.start] for k, v in enumerate(views)}
        todo = [dict(mat=c.index, uv0=uv0[i], uv1=uv1[i], grad=0.0, vc=(1, 1, 1, 1), cls="%s/%s" % (cls, c.kind)) for i, (c, uv, cls) in enumerate(c0[sl])]
        check(zoo.tables, todo, got, views, 0.0, tally)
    tally.report("four-gathers", zero_classes=("lattice", "clamp", "random"))


# ---- the material zoo -----------------------------------------------------------------------------------------------------------------------------
def _material_run(path, entries, views):
    rig = Rig(path)
    try:
        cases = tc.material_cases(entries)
        xyh, exp0, exp1, grads = [], [], [], []
        for n, (i, uv) in enumerate(cases):
            sx, sy = entries[i]["scale"]
            ox, oy = tc.node_origin(i)
            x, y = F32(ox + sx * (uv[0] - tc.UV_LO) / tc.UV_SPAN), F32(oy + sy * (uv[1] - tc.UV_LO) / tc.UV_SPAN)
            h = F32(2.0 ** (1.25 if n % 2 else -2.0) * 16.0)  # lod 1.25 / -2 of a 16-texel texture on an unscaled node under the identity transform
            xyh.append((x, y, h))
            e0, e1 = tc.expected_uv(i, x, y, (sx, sy))
            exp0.append(e0)
            exp1.append(e1)
            # texel density: uv area over world area of the triangle, square root (the reference renderer's computeTexelDensity, shaders/get_hit.h.slang:44-56)
            grads.append(tc.tex_grad_of(float(h), 1.0 / np.sqrt(sx * sy)))
        rays = make_rays(xyh)
        assert len(rays) <= SIDE * SIDE
        uv0, uv1 = device_uvs(rig, rays, [i for i, _ in cases], exp0, exp1, tc.PIXEL_ANGLE)
        got = render_views(rig, rays, views, tc.PIXEL_ANGLE)
        todo = [dict(mat=i, uv0=uv0[k], uv1=uv1[k], grad=grads[k], vc=entries[i]["vertex_colour"], cls="%s/%s" % (entries[i]["name"], "lod>0" if k % 2 else "lod<=0"))
                for k, (i, _) in enumerate(cases)]
        tally = Tally()
        check(rig.tables, todo, got, views, delta_lod_bound(), tally)
        return tally
    finally:
        rig.close()


def test_material_zoo_views(built, tmp_path):
    """Every map slot on its own, all of them together (SIMPLE is false), the specular-glossiness model, vertex colour, a slot without a valid
    texture (value 1), texture transforms (offset, scale, rotation over TEXCOORD_1), a non-uniformly scaled node (texel density): every field the
    views expose, and the guides of the default kernel."""
    path, entries = tc.build_material_zoo(str(tmp_path / "material_zoo.glb"))
    tally = _material_run(path, entries, tc.VIEWS_CORE + tc.VIEWS_EXT + ("GUIDE_ALBEDO", "GUIDE_NORMAL"))
    tally.report("material", zero_classes=tuple(e["name"] + "/lod<=0" for e in entries if "rotation" not in e["name"]))


def test_core_material_views_run_the_simple_kernels(built, tmp_path):
    """The core slots alone: no material of the scene has an extension lobe, so the SIMPLE instantiations of the shade kernels run."""
    path, entries = tc.build_material_zoo(str(tmp_path / "material_core.glb"), subset="core")
    tally = _material_run(path, entries, tc.VIEWS_CORE + ("GUIDE_ALBEDO", "GUIDE_NORMAL"))
    tally.report("core", zero_classes=tuple(e["name"] + "/lod<=0" for e in entries if "rotation" not in e["name"]))
