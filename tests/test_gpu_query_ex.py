"""Alpha-aware, face-culled and multi-hit ray queries (mi_pt_query_rays_ex, mi_pt_query_rays_device_ex, mi_pt_pick_ex; csrc/device/query.hip) on the
GPU, every case on the 8-wide tree and on the BVH2 (bvh=1).

 1. default options through the _ex calls return the bytes of the plain calls;
 2. CUTOFF (thresholds 0.5, 0.9) and STOCHASTIC (two seeds) against the float64 reference of tests/query_ex_util.py on four scenes; both trees
    return the same bytes; the same seed twice returns the same bytes; two seeds differ on the BLEND surfaces;
 3. CULL_MATERIAL against the reference, rays that start inside single-sided spheres, a mirrored render node;
 4. NEAREST_K with K = 1, 3, 8: the list check, K = 1 is CLOSEST, record j + 1 is the CLOSEST record with tMin = t[j], pre-split references listed once;
 5. the records after mi_pt_update_materials, a resident-mode variant switch and a refit equal a fresh instance's;
 6. the alpha-cut atrium (mi_scene_cut_alpha) against the uncut one under CUTOFF;
 7. mi_pt_pick_ex through a hole of the MASK card;
 8. refused arguments, invalid rays, no rays, an empty and a one-triangle scene;
 9. the device form with torch tensors (tests/query_ex_device_child.py).

Tolerances and ambiguous shares: query_ex_util (MEASURED / TOLERANCE, MAX_AMBIGUOUS_SHARE 2 %), measured on the CPU -- tests/test_query_ex_reference.py
re-measures them and runs the device's per-ray code through the same checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as pu
import query_ex_util as qx
import query_util as qu
from test_gpu_material_update import Holder, _tables
from test_gpu_query import CREATE_SWITCHES, _copy_desc, _environment, _holder
from test_gpu_refit import _matrix, _nodes, _rot, _set_matrix
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT, FRONT, INVALID = capi.MI_PT_HIT, capi.MI_PT_HIT_FRONT_FACE, capi.MI_PT_HIT_INVALID_RAY
ALPHA = {"opaque": qx.OPAQUE, "cutoff": qx.CUTOFF, "stochastic": qx.STOCHASTIC}
CULL = {"none": qx.CULL_NONE, "material": qx.CULL_MATERIAL}
# what the state-change tests compare with a fresh instance: every mode
EVERY_MODE = (dict(alpha="cutoff"), dict(alpha="cutoff", blend_threshold=0.9), dict(alpha="stochastic", seed=5), dict(cull="material"),
              dict(mode="any", alpha="cutoff", cull="material"), dict(mode="nearest_k", max_hits=4, alpha="cutoff", cull="material"))


def _options(mode=0, alpha=0, cull=0, max_hits=1, blend_threshold=0.5, seed=0, reserved=(0, 0)):
    o = capi.MiPtQueryOptions()
    o.mode, o.alpha, o.cull, o.maxHits, o.blendThreshold, o.seed = mode, alpha, cull, max_hits, blend_threshold, seed
    o.reserved[0], o.reserved[1] = reserved
    return o


def _raw(tr, rows, options, records_per_ray=1, fill=0):
    """mi_pt_query_rays_ex itself (PathTracer.query_rays takes the plain entry point for default options)."""
    rows = np.ascontiguousarray(rows, np.float32)
    hits = np.zeros((len(rows), records_per_ray), ptmod.HIT_DTYPE)
    hits.view(np.uint8)[:] = fill
    rc = tr._l.mi_pt_query_rays_ex(tr._p, rows.ctypes.data_as(C.POINTER(capi.MiPtRay)), len(rows), C.byref(options) if options is not None else None,
                                   hits.ctypes.data_as(C.POINTER(capi.MiPtRayHit)))
    return rc, hits


def _reference(case, **kw):
    key = tuple(sorted(kw.items()))
    if key not in case.refs:
        dec = qx.Decisions(case.pairs, case.sa, alpha=ALPHA[kw.get("alpha", "opaque")], cull=CULL[kw.get("cull", "none")],
                           blend_threshold=kw.get("blend_threshold", 0.5), seed=kw.get("seed", 0))
        case.refs[key] = qx.ReferenceEx(case.pairs, dec)
    return case.refs[key]


class Case:
    """One scene of the reference comparison: triangles, alpha side, rays, the float64 pairs, an instance per tree."""

    def __init__(self, name, directory):
        self.name = name
        self.scene = ptmod.Scene(qx.make_scene(name, directory))
        self.st = qu.SceneTris(self.scene)
        self.sa = qx.SceneAlpha(self.scene, self.st)
        self.rays = qx.make_rays_ex(self.st, self.sa)
        self.rows = qu.as_rows(self.rays)
        self.pairs = qu.Pairs(self.st, self.rays)
        self.refs = {}
        with _environment(CREATE_SWITCHES.get(name, {})):
            self.wide = ptmod.PathTracer(self.scene)
            self.bvh2 = ptmod.PathTracer(self.scene, bvh=1)
        self.trees = (("8-wide", self.wide), ("BVH2", self.bvh2))

    def both(self, **kw):
        """The records of both trees for one set of options -- the same bytes -- returned once."""
        a, b = self.wide.query_rays(self.rows, **kw), self.bvh2.query_rays(self.rows, **kw)
        assert a.tobytes() == b.tobytes(), (self.name, kw, int((a.view(np.uint8).reshape(-1, 64) != b.view(np.uint8).reshape(-1, 64)).any(1).sum()))
        return a

    def close(self):
        self.wide.close()
        self.bvh2.close()
        self.scene.close()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_query_ex")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, d)
        return made[name]
    yield get
    for c in made.values():
        c.close()


# ---- 1. defaults ------------------------------------------------------------------------------------------------------------------------------------
def test_default_options_return_the_plain_calls_bytes(cases):
    c = cases("mixed_alpha_glass")
    o = capi.MiPtQueryOptions()
    c.wide._l.mi_pt_default_query_options(C.byref(o))
    assert (o.mode, o.alpha, o.cull, o.maxHits, o.blendThreshold, o.seed, o.reserved[0], o.reserved[1]) == (0, 0, 0, 1, 0.5, 0, 0, 0)
    for label, tr in c.trees:
        for mode in ("closest", "any"):
            o.mode = capi.MI_PT_QUERY_ANY if mode == "any" else capi.MI_PT_QUERY_CLOSEST
            for max_hits in (1, 0):
                o.maxHits = max_hits
                rc, got = _raw(tr, c.rows, o, fill=0xAB)
                assert rc == 0 and got.tobytes() == tr.query_rays(c.rows, mode=mode).tobytes(), (label, mode, max_hits)
        tr.resize(128, 96)
        tr.set_frame_info(pu.Setup(c.scene.path, 128, 96, max_depth=2).frame_info)
        xy = np.stack([np.arange(16, 112) + 0.5, np.full(96, 50.25)], 1).astype(np.float32)
        o.mode, o.maxHits = capi.MI_PT_QUERY_CLOSEST, 1
        got = np.zeros(len(xy), ptmod.HIT_DTYPE)
        assert tr._l.mi_pt_pick_ex(tr._p, xy.ctypes.data_as(C.POINTER(C.c_float)), len(xy), C.byref(o), got.ctypes.data_as(C.POINTER(capi.MiPtRayHit))) == 0
        assert got.tobytes() == tr.pick(xy).tobytes() and (got["renderNode"] >= 0).any(), label


# ---- 2. alpha modes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qx.SCENES)
def test_alpha_modes_against_the_float64_reference(cases, name):
    c = cases(name)
    got = {}
    for label, kw in (("cutoff 0.5", dict(alpha="cutoff", blend_threshold=0.5)), ("cutoff 0.9", dict(alpha="cutoff", blend_threshold=0.9)),
                      ("stochastic 1", dict(alpha="stochastic", seed=1)), ("stochastic 99", dict(alpha="stochastic", seed=99))):
        ref = _reference(c, **kw)
        assert ref.ambiguous.mean() <= qx.MAX_AMBIGUOUS_SHARE, (name, label)  # (before anything of the GPU's is looked at)
        got[label] = c.both(**kw)
        assert got[label].shape == (len(c.rays),)
        qu.check_hits(c.st, c.rays, ref, got[label], *qx.TOLERANCE[name], what=name + ", " + label)
        assert c.wide.query_rays(c.rows, **kw).tobytes() == got[label].tobytes()  # the same call twice
        a = c.wide.query_rays(c.rows, mode="any", **kw)
        assert (((a["flags"] & HIT) != 0) == ((got[label]["flags"] & HIT) != 0)).all(), (name, label)
    opaque = c.wide.query_rays(c.rows)
    assert opaque.tobytes() != got["cutoff 0.5"].tobytes()  # the alpha test rejects what the plain query hits
    blend = np.array([n for n in np.unique(c.st.node) if c.sa.mode[c.st.node == n][0] == qx.ALPHA_BLEND])
    if len(blend):
        differ = (got["stochastic 1"]["renderNode"] != got["stochastic 99"]["renderNode"]) | (got["stochastic 1"]["triangle"] != got["stochastic 99"]["triangle"])
        on_blend = np.isin(got["stochastic 1"]["renderNode"], blend) | np.isin(got["stochastic 99"]["renderNode"], blend)
        assert (differ & on_blend).any(), name
        assert got["cutoff 0.5"].tobytes() != got["cutoff 0.9"].tobytes()
    else:
        assert got["stochastic 1"].tobytes() == got["stochastic 99"].tobytes() == got["cutoff 0.9"].tobytes()  # MASK alone: every mode follows the cutoff


# ---- 3. culling -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("mixed_alpha_glass", "zoo_vertex_streams"))
def test_cull_material_against_the_float64_reference(cases, name):
    c = cases(name)
    for label, kw in (("cull", dict(cull="material")), ("cutoff + cull", dict(alpha="cutoff", cull="material"))):
        ref = _reference(c, **kw)
        assert ref.ambiguous.mean() <= qx.MAX_AMBIGUOUS_SHARE
        got = c.both(**kw)
        qu.check_hits(c.st, c.rays, ref, got, *qx.TOLERANCE[name], what=name + ", " + label)
        h = (got["flags"] & HIT) != 0
        free = np.array([bool(c.sa.flags[c.st.node == n][0] & qx.INST_CULL_DISABLE) for n in got["renderNode"][h]])
        assert (((got["flags"][h] & FRONT) != 0) | free).all()  # a back face is returned only where culling is disabled
    assert c.both(cull="material").tobytes() != c.wide.query_rays(c.rows).tobytes()


def test_rays_from_inside_single_sided_spheres_leave_through_the_back_faces(cases):
    c = cases("mixed_alpha_glass")
    d = c.scene.desc.contents
    inside = [n for n in np.unique(c.st.node) if n > 0 and (c.sa.flags[c.st.node == n][0] & (qx.INST_FORCE_OPAQUE | qx.INST_CULL_DISABLE)) == qx.INST_FORCE_OPAQUE]
    assert len(inside) >= 2, inside  # the two opaque single-sided spheres
    rng = np.random.default_rng(3)
    rays, own = [], []
    for n in inside:
        centre = c.st.V[c.st.node == n].reshape(-1, 3).mean(0)
        dirs = rng.normal(size=(64, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        r = np.zeros(64, qu.RAY_DTYPE)
        r["origin"], r["direction"], r["tMin"], r["tMax"] = centre + 0.05 * rng.normal(size=(64, 3)), dirs, 0.0, np.inf
        rays.append(r)
        own += [n] * 64
    rays, own = np.concatenate(rays), np.array(own)
    pairs = qu.Pairs(c.st, rays)
    for label, tr in c.trees:
        plain = tr.query_rays(qu.as_rows(rays))
        assert (plain["renderNode"] == own).all() and ((plain["flags"] & FRONT) == 0).all(), label  # unculled: the sphere's own back face
        culled = tr.query_rays(qu.as_rows(rays), cull="material")
        assert (culled["renderNode"] != own).all() and (culled["renderNode"] >= 0).any() and (culled["renderNode"] < 0).any(), label
        ref = qx.ReferenceEx(pairs, qx.Decisions(pairs, c.sa, cull=qx.CULL_MATERIAL))
        qu.check_hits(c.st, rays, ref, culled, *qx.TOLERANCE[c.name], what="from inside the spheres, " + label)


def test_culling_under_a_mirroring_node_matrix(tmp_path):
    b = scenegen.GlbBuilder()
    mat = b.material(scenegen.lambert_material((0.7, 0.3, 0.3)))  # single sided
    pos, nrm, uv, idx = scenegen.uv_sphere(16, 8, 0.5)
    mesh = b.mesh([b.primitive(pos, idx, nrm, uv, material=mat)])
    b.node(mesh=mesh, translation=[-0.8, 0.0, 0.0])
    b.node(mesh=mesh, translation=[0.8, 0.1, 0.0], scale=[-1.0, 1.2, 1.0])  # det < 0: INST_FLIP_FACING
    b.camera_node((0.0, 0.5, 4.0), (0, 0, 0), yfov=0.7)
    scene = ptmod.Scene(b.save(str(tmp_path / "mirrored.glb")))
    st = qu.SceneTris(scene)
    sa = qx.SceneAlpha(scene, st)
    assert st.flip[st.node == 1].all() and not st.flip[st.node == 0].any()
    rays = qu.make_rays(st, n=512, seed=5)
    rng = np.random.default_rng(8)
    for k, centre in enumerate(((-0.8, 0.0, 0.0), (0.8, 0.1, 0.0))):  # rays from inside each sphere
        s = slice(256 + 64 * k, 256 + 64 * (k + 1))
        rays["origin"][s] = np.asarray(centre) + 0.05 * rng.normal(size=(64, 3))
    pairs = qu.Pairs(st, rays)
    ref = qx.ReferenceEx(pairs, qx.Decisions(pairs, sa, cull=qx.CULL_MATERIAL))
    assert ref.ambiguous.mean() <= qx.MAX_AMBIGUOUS_SHARE
    records = []
    for bvh in (0, 1):
        tr = ptmod.PathTracer(scene, bvh=bvh)
        got = tr.query_rays(qu.as_rows(rays), cull="material")
        qu.check_hits(st, rays, ref, got, *qu.TOLERANCE["animated"], what="mirrored node, bvh %d" % bvh)
        h = (got["flags"] & HIT) != 0
        assert ((got["flags"][h] & FRONT) != 0).all() and (got["renderNode"][h] == 0).any() and (got["renderNode"][h] == 1).any()
        plain = tr.query_rays(qu.as_rows(rays))
        back = ((plain["flags"] & HIT) != 0) & ((plain["flags"] & FRONT) == 0)
        assert (plain["renderNode"][back] == 0).any() and (plain["renderNode"][back] == 1).any()  # from inside, both spheres show their backs
        records.append(got)
        tr.close()
    assert records[0].tobytes() == records[1].tobytes()
    scene.close()


# ---- 4. the K nearest -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qx.SCENES)
def test_nearest_k_lists(cases, name):
    c = cases(name)
    kw = dict(alpha="cutoff", cull="material")
    ref = _reference(c, **kw)
    closest = c.both(**kw)
    if name == "atrium_sliver":
        slots = c.wide.stats()["bvhTriangleCount"]
        assert slots > c.scene.num_triangles == len(c.st), (slots, c.scene.num_triangles)  # the tree really holds pre-split references
    for k in (1, 3, 8):
        lists = c.both(mode="nearest_k", max_hits=k, **kw)
        assert lists.shape == (len(c.rays), k)
        qx.check_lists(c.st, c.rays, ref, lists, k, qx.TOLERANCE[name][0], what=name)  # (no triangle twice: pre-split references are listed once)
        assert lists[:, 0].tobytes() == closest.tobytes(), k  # the nearest of the K is the CLOSEST record
        if k == 1:
            continue
        # where t[j + 1] > t[j] strictly, record j + 1 is the CLOSEST record of the same ray with tMin = t[j]
        for j in range(min(k, 4) - 1):
            nxt = c.rays.copy()
            nxt["tMin"] = lists["t"][:, j]
            after = c.wide.query_rays(qu.as_rows(nxt), **kw)
            strict = ((lists["flags"][:, j + 1] & HIT) != 0) & (lists["t"][:, j + 1] > lists["t"][:, j])
            assert strict.any() or j > 0, (name, k, j)  # (every scene has rays with a second hit)
            assert after[strict].tobytes() == lists[:, j + 1][strict].tobytes(), (name, k, j)
            ends = ((lists["flags"][:, j] & HIT) != 0) & ((lists["flags"][:, j + 1] & HIT) == 0)
            assert (after["flags"][ends] == 0).all()  # the list ended: nothing lies behind its last record
    # the plain rules with K > 1 (every triangle opaque, no culling)
    plain = c.both(mode="nearest_k", max_hits=4)
    assert plain[:, 0].tobytes() == c.wide.query_rays(c.rows).tobytes()
    qx.check_lists(c.st, c.rays, _reference(c), plain, 4, qx.TOLERANCE[name][0], what=name + ", opaque")


# ---- 5. the current state -------------------------------------------------------------------------------------------------------------------------------
def _every_mode(tr, rows):
    """The records of every mode as bytes; of ANY, whose choice of triangle is unspecified, the hit flags alone."""
    out = []
    for kw in EVERY_MODE:
        got = tr.query_rays(rows, **kw)
        out.append(((got["flags"] & HIT) != 0).tobytes() if kw.get("mode") == "any" else got.tobytes())
    return out


def _fresh(scene_or_holder, rows, **create):
    fresh = ptmod.PathTracer(scene_or_holder, **create)
    out = _every_mode(fresh, rows)
    fresh.close()
    return out


@pytest.mark.parametrize("bvh", [0, 1])
def test_records_after_a_material_update_equal_a_fresh_instances(cases, bvh):
    c = cases("mixed_alpha_glass")
    d = c.scene.desc.contents
    mask = [m for m in range(d.numMaterials) if d.materials[m].alphaMode == qx.ALPHA_MASK]
    blend = [m for m in range(d.numMaterials) if d.materials[m].alphaMode == qx.ALPHA_BLEND and d.materials[m].pbrBaseColorTexture > 0]
    assert len(mask) == 1 and len(blend) == 1
    tr = ptmod.PathTracer(c.scene, bvh=bvh)
    before = _every_mode(tr, c.rows)
    builds = tr.accel_info()["builds"]
    mats, infos = _tables(c.scene)
    mats[mask[0]].alphaCutoff = 0.3
    mats[blend[0]].pbrBaseColorFactor[3] = 0.5
    tr.update_materials(mats, len(mats), infos, len(infos))
    # on the 8-wide tree in place -- the patch kernel rewrote the alpha records; the BVH2 walk rebuilds on an alpha change (include/mi_pt.h)
    assert tr.accel_info()["builds"] == builds + bvh
    after = _every_mode(tr, c.rows)
    want = _fresh(Holder(c.scene, mats, infos), c.rows, bvh=bvh)
    for kw, a, w, b0 in zip(EVERY_MODE, after, want, before):
        assert a == w, kw
        if kw.get("alpha") == "cutoff" and kw.get("mode") != "any":
            assert a != b0, kw  # the new cutoff and factor show
    tr.close()


def test_records_after_a_resident_variant_switch_equal_a_fresh_instances(tmp_path):
    scene = ptmod.Scene(scenegen.scene_variants(str(tmp_path / "variants.glb")))
    d = scene.desc.contents
    st = qu.SceneTris(scene)
    rows = qu.as_rows(qu.make_rays(st, n=2048, seed=11))
    tr = ptmod.PathTracer(scene)
    tr.set_accel_update("refit")
    tr.set_accel_resident(True)
    assert tr.accel_resident_info()["inForce"] == 1
    before = _every_mode(tr, rows)
    assert before == _fresh(scene, rows)
    patches = tr.accel_resident_info()["materialPatches"]
    assert scene.set_variant(1) > 0  # "cutout": sphere A takes the alpha-MASK material -- the scene's first alpha-tested triangles
    tr.update_render_nodes(d.renderNodes, d.numRenderNodes, d.renderNodeVisible)
    assert tr.accel_resident_info()["materialPatches"] == patches + 1
    after = _every_mode(tr, rows)
    assert after == _fresh(scene, rows)
    cut = EVERY_MODE.index(dict(alpha="cutoff"))
    assert after[cut] != before[cut] and after[cut] != tr.query_rays(rows).tobytes()  # rays pass through the cut-out now
    tr.close()
    scene.close()


def test_records_after_a_refit_equal_a_fresh_instances(tmp_path):
    st = pu.Setup(scenegen.scene_animated(str(tmp_path / "animated.glb")), 128, 96, max_depth=2)
    nodes, n = _nodes(st.scene)
    tr = ptmod.PathTracer(st.scene)
    tr.set_accel_update("refit")
    rows = qu.as_rows(qu.make_rays(qu.SceneTris(st.scene), n=2048, seed=11))
    before = _every_mode(tr, rows)
    _set_matrix(nodes[1], _rot(1, 0.4, (0.2, 0.3, 0.0)) @ _matrix(nodes[1]))
    tr.update_render_nodes(nodes, n, st.scene.desc.contents.renderNodeVisible)
    assert tr.accel_info()["lastUpdate"] == capi.MI_PT_ACCEL_LAST_REFIT
    after = _every_mode(tr, rows)
    assert after == _fresh(st.scene, rows)
    assert all(a != b for a, b in zip(after, before))
    tr.close()


# ---- 6. alpha-cut geometry ------------------------------------------------------------------------------------------------------------------------------
def test_cutoff_on_the_alpha_cut_atrium_agrees_with_the_uncut_one(cases, tmp_path):
    c = cases("atrium_sliver")
    ref = _reference(c, alpha="cutoff")
    uncut = c.both(alpha="cutoff")
    scene = ptmod.Scene(c.scene.path)
    assert scene.cut_alpha() > 0
    st = qu.SceneTris(scene)
    sa = qx.SceneAlpha(scene, st)
    assert (sa.flags & qx.INST_FORCE_OPAQUE)[sa.mode == qx.ALPHA_MASK].any()  # triangles the cut classified opaque: accepted untested
    pairs = qu.Pairs(st, c.rays)
    ref_cut = qx.ReferenceEx(pairs, qx.Decisions(pairs, sa, alpha=qx.CUTOFF))
    tol_t, tol_b = qx.TOLERANCE[c.name]
    for bvh in (0, 1):
        tr = ptmod.PathTracer(scene, bvh=bvh)
        cut = tr.query_rays(c.rows, alpha="cutoff")
        tr.close()
        qu.check_hits(st, c.rays, ref_cut, cut, tol_t, tol_b, what="alpha-cut atrium, bvh %d" % bvh)
        s = ~ref.ambiguous & ~ref_cut.ambiguous
        assert s.mean() > 0.97
        # the references agree -- the cut drops only what cannot pass (t to the rounding of the cut's float32 vertices)
        assert (ref.hit[s] == ref_cut.hit[s]).all()
        assert (np.abs(ref.t[s & ref.hit] - ref_cut.t[s & ref.hit]) <= tol_t * np.maximum(1.0, ref.t[s & ref.hit])).all()
        hit = (uncut["flags"] & HIT) != 0
        assert (((cut["flags"] & HIT) != 0)[s] == hit[s]).all()
        both = s & hit
        assert (cut["renderNode"][both] == uncut["renderNode"][both]).all()
        assert (np.abs(cut["t"][both].astype(np.float64) - uncut["t"][both]) / np.maximum(1.0, uncut["t"][both]) <= 2 * tol_t).all()
    scene.close()


# ---- 7. picking -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", [0, 1])
def test_pick_ex_through_a_hole_of_the_mask_card(cases, bvh):
    c = cases("mixed_alpha_glass")
    w, h = 160, 120
    setup = pu.Setup(c.scene.path, w, h, max_depth=2)
    tr = ptmod.PathTracer(c.scene, bvh=bvh)
    tr.resize(w, h)
    tr.set_frame_info(setup.frame_info)
    ys, xs = np.mgrid[0:h, 0:w]
    xy = np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], 1).astype(np.float32)[::5]  # 3840 positions
    card = int([n for n in np.unique(c.st.node) if c.sa.mode[c.st.node == n][0] == qx.ALPHA_MASK][0])
    opaque, seen = tr.pick(xy), tr.pick(xy, alpha="cutoff", cull="material")
    assert opaque.tobytes() == tr.pick(xy, mode="nearest_k", max_hits=1).reshape(-1).tobytes()
    holes = np.nonzero((opaque["renderNode"] == card) & (seen["renderNode"] != card))[0]
    solid = np.nonzero((opaque["renderNode"] == card) & (seen["renderNode"] == card))[0]
    assert len(holes) > 5 and len(solid) > 5, (len(holes), len(solid))  # OPAQUE names the card; CUTOFF names what lies behind its holes
    behind = holes[seen["renderNode"][holes] >= 0]
    assert len(behind) > 0 and (seen["t"][behind] > opaque["t"][behind]).all()
    # on the card's solid part both name the same triangle (mi_pt_pick_ex forms its rays in a kernel of its own under non-default options:
    # the camera ray may round differently in the last place there, so t is compared to the scene's tolerance, not bit for bit)
    for f in ("renderNode", "renderPrimID", "triangle", "materialID", "flags"):
        assert (seen[f][solid] == opaque[f][solid]).all(), f
    assert (np.abs(seen["t"][solid] - opaque["t"][solid]) <= qx.TOLERANCE[c.name][0] * np.maximum(1.0, opaque["t"][solid])).all()
    # the same camera rays through mi_pt_query_rays_ex: the eye, and the direction to the picked position
    cam = c.scene.camera(0)
    eye = np.array(cam.eye[:], np.float64)
    rays = np.zeros(len(holes), qu.RAY_DTYPE)
    dirs = opaque["position"][holes].astype(np.float64) - eye
    rays["origin"], rays["direction"], rays["tMin"], rays["tMax"] = eye, dirs / np.linalg.norm(dirs, axis=1, keepdims=True), 0.0, np.inf
    for kw, want in ((dict(alpha="opaque", cull="none", max_hits=1, mode="nearest_k"), opaque[holes]), (dict(alpha="cutoff", cull="material"), seen[holes])):
        got = tr.query_rays(qu.as_rows(rays), **kw).reshape(-1)
        same = (got["renderNode"] == want["renderNode"]) & (got["triangle"] == want["triangle"])
        assert same.mean() > 0.9, kw  # (the rebuilt direction differs in the last place: a ray at an edge may take the neighbour)
        hit = same & (want["renderNode"] >= 0)
        assert (np.abs(got["t"][hit] - want["t"][hit]) <= 1e-4 * np.maximum(1.0, want["t"][hit])).all()
    # what is under the cursor, and behind that
    under = tr.pick(xy[holes], mode="nearest_k", max_hits=3)
    assert under.shape == (len(holes), 3) and (under["renderNode"][:, 0] == card).all() and (under["triangle"][:, 0] == opaque["triangle"][holes]).all()
    second = under["renderNode"][:, 1][seen["renderNode"][holes] >= 0]
    assert (second >= 0).all()  # something lies behind the card wherever the alpha-aware pick found something
    tr.close()


# ---- 8. errors and edges --------------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_output_untouched(cases):
    c = cases("mixed_alpha_glass")
    tr, rows = c.wide, c.rows[:8]
    nan = float("nan")
    refused = [dict(mode=3), dict(mode=-1), dict(alpha=3), dict(alpha=-1), dict(cull=2), dict(cull=-1), dict(mode=2, max_hits=0), dict(mode=2, max_hits=9),
               dict(mode=0, max_hits=2), dict(mode=1, max_hits=-1), dict(alpha=1, blend_threshold=0.0), dict(alpha=1, blend_threshold=1.5),
               dict(alpha=1, blend_threshold=-0.5), dict(alpha=1, blend_threshold=nan), dict(reserved=(1, 0)), dict(reserved=(0, -7))]
    for kw in refused:
        rc, hits = _raw(tr, rows, _options(**kw), records_per_ray=8, fill=0xAB)
        assert rc == -1 and (hits.view(np.uint8) == 0xAB).all(), kw
        assert tr._l.mi_pt_query_rays_device_ex(tr._p, None, 0, C.byref(_options(**kw)), None, None) == -1, kw
        assert tr._l.mi_pt_pick_ex(tr._p, None, 0, C.byref(_options(**kw)), None) == -1, kw
    rc, hits = _raw(tr, rows, None, fill=0xAB)
    assert rc == -1 and (hits.view(np.uint8) == 0xAB).all()  # NULL options
    ok = _options(mode=2, max_hits=4, alpha=1)
    P, H = C.POINTER(capi.MiPtRay), C.POINTER(capi.MiPtRayHit)
    assert tr._l.mi_pt_query_rays_ex(tr._p, None, 4, C.byref(ok), None) == -1
    assert tr._l.mi_pt_query_rays_ex(tr._p, rows.ctypes.data_as(P), -1, C.byref(ok), hits.ctypes.data_as(H)) == -1
    assert tr._l.mi_pt_query_rays_ex(None, rows.ctypes.data_as(P), 4, C.byref(ok), hits.ctypes.data_as(H)) == -1
    assert tr._l.mi_pt_query_rays_device_ex(tr._p, None, 4, C.byref(ok), None, None) == -1
    assert tr._l.mi_pt_query_rays_device_ex(tr._p, C.c_void_p(rows.ctypes.data + 4), 1, C.byref(ok), C.c_void_p(hits.ctypes.data), None) == -1  # alignment
    assert tr._l.mi_pt_pick_ex(tr._p, None, 4, C.byref(ok), None) == -1
    # threshold values outside (0, 1] are fine where CUTOFF is not asked for; numRays == 0 succeeds
    rc, _ = _raw(tr, rows, _options(alpha=2, blend_threshold=7.0))
    assert rc == 0
    assert tr._l.mi_pt_query_rays_ex(tr._p, None, 0, C.byref(ok), None) == 0 and tr._l.mi_pt_query_rays_device_ex(tr._p, None, 0, C.byref(ok), None, None) == 0
    assert tr.query_rays(c.rows[:0], mode="nearest_k", max_hits=4).shape == (0, 4)
    with pytest.raises(ValueError):
        tr.query_rays(rows, mode="nearest_k", max_hits=9)
    with pytest.raises(ptmod.MiError):
        tr.query_rays(rows, alpha="cutoff", blend_threshold=0.0)


def test_invalid_rays_batch_sizes_and_memory_under_k_4(cases):
    c = cases("mixed_alpha_glass")
    kw = dict(mode="nearest_k", max_hits=4, alpha="cutoff", cull="material")
    for label, tr in c.trees:
        whole = tr.query_rays(c.rows, **kw)
        for n in (1, 63, 65, 257):
            assert tr.query_rays(c.rows[:n], **kw).tobytes() == whole[:n].tobytes(), (label, n)
        mixed = c.rows[:257].copy()
        bad = {3: (0, np.nan), 64: (4, np.inf), 130: (3, np.nan), 256: (7, np.nan)}
        for i, (col, val) in bad.items():
            mixed[i, col] = val
        mixed[10, 4:7] = 0.0
        idx = np.array(sorted(list(bad) + [10]))
        got = tr.query_rays(mixed, **kw)
        assert (got["flags"][idx, 0] == INVALID).all() and (got["flags"][idx, 1:] == 0).all() and (got["renderNode"][idx] == -1).all()
        z = got[idx].copy()
        z["flags"], z["renderNode"] = 0, 0
        assert not z.view(np.uint8).any()
        good = np.setdiff1d(np.arange(257), idx)
        assert got[good].tobytes() == whole[:257][good].tobytes(), label
    # the staging of the host form: numRays x K records, counted in rendererBytes
    tr = ptmod.PathTracer(c.scene)
    m0 = tr.memory()["rendererBytes"]
    tr.query_rays(c.rows[:300], **kw)
    assert tr.memory()["rendererBytes"] - m0 == 300 * (32 + 4 * 64)
    tr.query_rays(c.rows[:300], alpha="cutoff")
    assert tr.memory()["rendererBytes"] - m0 == 300 * (32 + 4 * 64)
    tr.close()


@pytest.mark.parametrize("bvh", [0, 1])
def test_empty_and_one_triangle_scenes(cases, bvh):
    c = cases("mixed_alpha_glass")
    rows = c.rows[:300]
    desc = _copy_desc(c.scene)
    hidden = (C.c_uint8 * desc.numRenderNodes)()
    desc.renderNodeVisible = C.cast(hidden, C.POINTER(C.c_uint8))
    tr = ptmod.PathTracer(_holder(desc, [hidden]), bvh=bvh)
    assert tr.stats()["bvhTriangleCount"] == 0
    for kw in EVERY_MODE:
        m = tr.query_rays(rows, **kw)
        assert (m["renderNode"] == -1).all() and (m["flags"] == 0).all() and not m["position"].any(), kw
    tr.close()
    # one triangle: the first triangle of the MASK card, alone
    card = int([n for n in np.unique(c.st.node) if c.sa.mode[c.st.node == n][0] == qx.ALPHA_MASK][0])
    desc = _copy_desc(c.scene)
    node = (capi.MiGltfRenderNode * 1)()
    C.memmove(node, C.byref(desc.renderNodes[card]), C.sizeof(node))
    prims = (capi.MiPtRenderPrimitive * desc.numRenderPrimitives)()
    C.memmove(prims, desc.renderPrimitives, C.sizeof(prims))
    prims[node[0].renderPrimID].triangleCount = 1
    prims[node[0].renderPrimID].opaqueTriangleCount = 0
    desc.renderNodes, desc.numRenderNodes, desc.renderNodeVisible, desc.renderPrimitives = node, 1, None, prims
    holder = _holder(desc, [node, prims])
    tr = ptmod.PathTracer(holder, bvh=bvh)
    assert tr.stats()["bvhTriangleCount"] == 1
    one = qu.SceneTris(holder)
    sa = qx.SceneAlpha(holder, one)
    assert len(one) == 1 and sa.tested.all()
    rng = np.random.default_rng(4)
    r1, r2 = np.sqrt(rng.uniform(size=256)), rng.uniform(size=256)
    p = one.V[0, 0] * (1 - r1)[:, None] + one.V[0, 1] * (r1 * (1 - r2))[:, None] + one.V[0, 2] * (r1 * r2)[:, None]
    n = np.cross(one.e1[0], one.e2[0])
    o = p + (n / np.linalg.norm(n)) * np.where(np.arange(256) % 2 == 0, 1.5, -1.5)[:, None] + 0.2 * rng.normal(size=(256, 3))
    rays = np.zeros(256, qu.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tMin"], rays["tMax"] = o, (p - o) / np.linalg.norm(p - o, axis=1, keepdims=True), 0.0, np.inf
    pairs = qu.Pairs(one, rays)
    assert (tr.query_rays(qu.as_rows(rays))["renderNode"] == 0).mean() > 0.9
    for kw, dec in ((dict(alpha="cutoff"), dict(alpha=qx.CUTOFF)), (dict(alpha="stochastic", seed=3), dict(alpha=qx.STOCHASTIC, seed=3)),
                    (dict(alpha="cutoff", cull="material"), dict(alpha=qx.CUTOFF, cull=qx.CULL_MATERIAL))):
        ref = qx.ReferenceEx(pairs, qx.Decisions(pairs, sa, **dec))
        got = tr.query_rays(qu.as_rows(rays), **kw)
        qu.check_hits(one, rays, ref, got, *qx.TOLERANCE[c.name], what="one triangle, bvh %d, %s" % (bvh, kw))
        lists = tr.query_rays(qu.as_rows(rays), mode="nearest_k", max_hits=8, **kw)
        assert lists[:, 0].tobytes() == got.tobytes() and (lists["flags"][:, 1:] == 0).all()
        assert tr.query_rays(qu.as_rows(rays), mode="any", **kw).tobytes() == got.tobytes()
    tr.close()


# ---- 9. the device form ---------------------------------------------------------------------------------------------------------------------------------
def test_device_form_with_torch_tensors(tmp_path):
    """In a process of its own (tests/query_ex_device_child.py), torch imported first, as tests/test_gpu_query.py explains for the plain form."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "query_ex_device_child.py"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "QUERY_EX_DEVICE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
