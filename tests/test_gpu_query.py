"""Ray queries and picking against the resident scene (mi_pt_query_rays, mi_pt_query_rays_device, mi_pt_pick; csrc/device/query.hip) on the GPU.

1. pick at every pixel centre returns the render node the selection pass of a first frame wrote (perspective, orthographic, BVH2);
2. closest hits against a float64 brute force over the scene description (tests/query_util.py), on four scenes -- alpha-tested and
   transmissive surfaces hit as opaque, pre-split references in the tree;
3. the tree does not matter: the 8-wide tree and the BVH2 return the same bytes; ANY agrees with CLOSEST on hit / miss; the ray interval;
4. the query sees the current state: deformation, node moves, resident-mode visibility and material ids -- the bytes of a fresh instance;
5. an empty scene, a one-triangle scene, partial waves and blocks, invalid rays among valid ones;
6. the device form (torch tensors), and a query between queued frames;
7. memory and counters.

Tolerances and ambiguous shares: query_util.MEASURED / TOLERANCE, measured on the CPU (tests/test_query_reference.py re-measures them): per scene
8 x the largest difference between the float32 ray / triangle test and float64 on the test's own unambiguous pairs -- animated t 3.4e-7 /
barycentrics 1.1e-5, variants 1.0e-6 / 5.9e-5, mixed alpha + glass 8.6e-7 / 3.0e-5, sliver atrium 7.3e-5 / 1.9e-4; ambiguous shares (seed 7, 2048
rays, DELTA 1e-4) 0.05 % / 0.00 % / 0.00 % / 0.20 %, cap 1 %."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import deform_util as du
import parity_util as pu
import query_util as qu
from test_gpu_refit import _matrix, _nodes, _render, _rot, _set_matrix, _tracer
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 128, 96
HIT, FRONT, INVALID = capi.MI_PT_HIT, capi.MI_PT_HIT_FRONT_FACE, capi.MI_PT_HIT_INVALID_RAY
SCENES = sorted(qu.MEASURED)


@contextlib.contextmanager
def _environment(values):
    """MI_PT_* switches are read once, in mi_pt_create: set for the instances created inside, restored afterwards."""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# The sliver atrium at this detail stays below the share of large triangles from which the builder pre-splits by default (MI_PT_SPLIT_MIN_SHARE,
# 0.1: its tree holds one slot per triangle, as tests/test_gpu_resident.py notes).  The comparison wants pre-split references in the tree, so
# its instances are created with the gate open (0 = always split what exceeds MI_PT_SPLIT x the mean box area); the test asserts that they are there.
CREATE_SWITCHES = {"atrium_sliver": {"MI_PT_SPLIT_MIN_SHARE": "0"}}


class Case:
    """One scene of the reference comparison: its triangles, rays, float64 reference, and the closest-mode records of both trees."""

    def __init__(self, name, directory):
        self.name = name
        self.path = qu.make_scene(name, directory)
        self.scene = ptmod.Scene(self.path)
        self.st = qu.SceneTris(self.scene)
        self.rays = qu.make_rays(self.st)
        self.pairs = qu.Pairs(self.st, self.rays)
        self.ref = qu.Reference(self.pairs)
        self.share = float(self.ref.ambiguous.mean())
        with _environment(CREATE_SWITCHES.get(name, {})):
            self.wide = ptmod.PathTracer(self.scene)
            self.bvh2 = ptmod.PathTracer(self.scene, bvh=1)
        self.closest = self.wide.query_rays(qu.as_rows(self.rays))
        self.closest2 = self.bvh2.query_rays(qu.as_rows(self.rays))

    def close(self):
        self.wide.close()
        self.bvh2.close()
        self.scene.close()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_query")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, d)
        return made[name]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def animated(tmp_path_factory):
    return scenegen.scene_animated(str(tmp_path_factory.mktemp("gpu_query_anim") / "animated.glb"))


def _centres():
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], 1).astype(np.float32)


# ---- 1. against the selection pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera,bvh", [("perspective", 0), ("orthographic", 0), ("perspective", 1)])
def test_pick_at_every_pixel_centre_is_the_selection_image(animated, camera, bvh):
    scene = ptmod.Scene(animated)
    cam = scene.camera(0)
    if camera == "orthographic":
        cam.orthographic, cam.xmag, cam.ymag = 1, 4.0, 3.0
    st = pu.Setup(animated, W, H, max_depth=2, camera=cam)
    tr = _tracer(st, bvh=bvh)
    with pytest.raises(ptmod.MiError):
        tr.pick([(float(W), 1.0)])  # outside the image
    _render(tr, st, frames=1)
    sel = tr.read_selection()
    hits = tr.pick(_centres())
    assert len(hits) == W * H == 12288
    got = (hits["renderNode"] + 1).reshape(H, W)
    assert (got == sel.astype(np.int64)).all(), int((got != sel).sum())
    assert 0.05 < (sel > 0).mean() < 1.0 and len(np.unique(sel)) > 2  # the camera sees several nodes and some background
    assert (((hits["flags"] & HIT) != 0) == (hits["renderNode"] >= 0)).all()
    # a camera ray has unit direction: the distance is t, and the position lies on the ray
    h = hits[hits["renderNode"] >= 0]
    assert (h["t"] > 0).all() and np.isfinite(h["position"]).all()
    one = tr.pick((W / 2 + 0.5, H / 2 + 0.5))
    assert one.tobytes() == hits[(H // 2) * W + W // 2].tobytes()
    tr.close()
    scene.close()


def test_pick_before_resize_is_a_state_error(animated):
    scene = ptmod.Scene(animated)
    tr = ptmod.PathTracer(scene)
    with pytest.raises(ptmod.MiError):
        tr.pick([(1.5, 1.5)])
    tr.close()
    scene.close()


# ---- 2. against float64 brute force --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_closest_hits_against_float64_brute_force(cases, name):
    c = cases(name)
    print("QUERY", name, "triangles", len(c.st), "ambiguous share %.4f %%" % (100 * c.share))
    assert c.share <= qu.MAX_AMBIGUOUS_SHARE  # (before anything of the GPU's is looked at)
    if name == "atrium_sliver":
        slots = c.wide.stats()["bvhTriangleCount"]
        print("QUERY", name, "triangle slots", slots, "BVH2", c.bvh2.stats()["bvhTriangleCount"])
        assert slots > c.scene.num_triangles == len(c.st), (slots, c.scene.num_triangles)  # pre-split references really are in the tree
    if name == "mixed_alpha_glass":
        # alpha-tested and transmissive nodes are hit like any other: each of them is some ray's closest hit
        d = c.scene.desc.contents
        non_opaque = {n for n in range(d.numRenderNodes)
                      if d.materials[max(0, d.renderNodes[n].materialID)].alphaMode != 0 or d.materials[max(0, d.renderNodes[n].materialID)].transmissionFactor > 0}
        assert len(non_opaque) >= 4 and non_opaque <= set(c.closest["renderNode"].tolist()), (non_opaque, set(c.closest["renderNode"].tolist()))
    qu.check_hits(c.st, c.rays, c.ref, c.closest, *qu.TOLERANCE[name], what=name)


# ---- 3. the tree does not matter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_both_trees_return_the_same_bytes_and_any_agrees_with_closest(cases, name):
    c = cases(name)
    assert c.closest.tobytes() == c.closest2.tobytes(), int((c.closest.view(np.uint8).reshape(-1, 64) != c.closest2.view(np.uint8).reshape(-1, 64)).any(1).sum())
    hit = (c.closest["flags"] & HIT) != 0
    for tr in (c.wide, c.bvh2):
        a = tr.query_rays(qu.as_rows(c.rays), mode="any")
        assert (((a["flags"] & HIT) != 0) == hit).all()
        assert (a["renderNode"][~hit] == -1).all() and (a["flags"][~hit] == 0).all()
        assert (a["t"][hit] >= c.closest["t"][hit]).all()  # whichever triangle ANY describes, it is not nearer than the closest
    # tMax at half the closest distance: nothing is hit
    short = c.rays.copy()
    short["tMax"] = np.where(hit, 0.5 * c.closest["t"], np.inf).astype(np.float32)
    for tr in (c.wide, c.bvh2):
        for mode in ("closest", "any"):
            m = tr.query_rays(qu.as_rows(short), mode=mode)
            assert (m["flags"][hit] == 0).all() and (m["renderNode"][hit] == -1).all(), mode
    # tMin just past the closest distance: the next surface, as the brute force says
    past = c.rays.copy()
    # ("just past": 2.5 DELTA x max(1, t) -- beyond the band in which the reference calls a surface at an end of the interval ambiguous)
    past["tMin"] = np.where(hit, c.closest["t"] + 2.5 * qu.DELTA * np.maximum(1.0, c.closest["t"]), 0.0).astype(np.float32)
    ref = qu.Reference(c.pairs, tmin=past["tMin"].astype(np.float64))
    second = c.wide.query_rays(qu.as_rows(past))
    assert second.tobytes() == c.bvh2.query_rays(qu.as_rows(past)).tobytes()
    qu.check_hits(c.st, past, ref, second, *qu.TOLERANCE[name], what=name + ", tMin past the closest hit")
    changed = hit & ((second["renderNode"] != c.closest["renderNode"]) | (second["triangle"] != c.closest["triangle"]))
    assert changed.sum() == hit.sum() > 0  # changed or disappeared: the closest triangle itself lies in front of tMin now
    assert ref.ambiguous.mean() <= 2 * qu.MAX_AMBIGUOUS_SHARE, ref.ambiguous.mean()  # (the comparison is not hollow)


# ---- 4. the query sees the current state ---------------------------------------------------------------------------------------------------------
def _rays_for(scene, n=2048, seed=11):
    st = qu.SceneTris(scene)
    return st, qu.make_rays(st, n=n, seed=seed)


def _fresh_bytes(scene_or_holder, rays):
    fresh = ptmod.PathTracer(scene_or_holder)
    out = fresh.query_rays(qu.as_rows(rays))
    fresh.close()
    return out


def test_query_after_deformation_under_refit(tmp_path):
    st = pu.Setup(scenegen.scene_skinned(str(tmp_path / "skinned.glb")), W, H, max_depth=2)
    tr = ptmod.PathTracer(st.scene)
    tr.set_deformation(st.scene)
    tr.set_accel_update("refit")
    _, rays = _rays_for(st.scene)
    rest = tr.query_rays(qu.as_rows(rays))
    assert rest.tobytes() == _fresh_bytes(st.scene, rays).tobytes()
    for time in (0.6, 1.4):
        assert st.scene.update_animation(0, time)
        tr.update_from_scene(st.scene)
        assert tr.accel_info()["lastUpdate"] == capi.MI_PT_ACCEL_LAST_REFIT
        got = tr.query_rays(qu.as_rows(rays))
        streams = {p.renderPrimID: tr.read_vertices(p.renderPrimID) for p in du.prims(st.scene.deformation)}
        holder, keep = du.posed_desc(st.scene, streams)
        assert got.tobytes() == _fresh_bytes(holder, rays).tobytes(), time
        assert got.tobytes() != rest.tobytes()
    tr.close()


def test_query_after_a_node_move_under_refit(animated):
    st = pu.Setup(animated, W, H, max_depth=2)
    nodes, n = _nodes(st.scene)
    tr = ptmod.PathTracer(st.scene)
    tr.set_accel_update("refit")
    _, rays = _rays_for(st.scene)
    before = tr.query_rays(qu.as_rows(rays))
    _set_matrix(nodes[1], _rot(1, 0.4, (0.2, 0.3, 0.0)) @ _matrix(nodes[1]))
    tr.update_render_nodes(nodes, n, st.scene.desc.contents.renderNodeVisible)
    assert tr.accel_info()["lastUpdate"] == capi.MI_PT_ACCEL_LAST_REFIT
    got = tr.query_rays(qu.as_rows(rays))
    assert got.tobytes() == _fresh_bytes(st.scene, rays).tobytes()
    assert got.tobytes() != before.tobytes()
    # ... and against the float64 reference of the moved scene
    moved = qu.SceneTris(st.scene)
    qu.check_hits(moved, rays, qu.Reference(qu.Pairs(moved, rays)), got, *qu.TOLERANCE["animated"], what="animated, node 1 moved")
    tr.close()


def test_query_in_resident_mode_after_hiding_a_node_and_changing_material_ids(tmp_path):
    st = pu.Setup(scenegen.scene_variants(str(tmp_path / "variants.glb")), W, H, max_depth=2)
    d = st.scene.desc.contents
    tr = ptmod.PathTracer(st.scene)
    tr.set_accel_update("refit")
    tr.set_accel_resident(True)
    assert tr.accel_resident_info()["inForce"] == 1
    _, rays = _rays_for(st.scene)
    before = tr.query_rays(qu.as_rows(rays))
    nodes_hit, counts = np.unique(before["renderNode"][before["renderNode"] >= 0], return_counts=True)
    hide = int(nodes_hit[np.argmax(counts)])  # the node most rays end on
    refits = tr.accel_resident_info()["visibilityRefits"]
    d.renderNodeVisible[hide] = 0
    tr.update_render_nodes(d.renderNodes, d.numRenderNodes, d.renderNodeVisible)
    info = tr.accel_resident_info()
    assert info["visibilityRefits"] == refits + 1 and info["hiddenTriangles"] > 0 and tr.accel_info()["lastUpdate"] == capi.MI_PT_ACCEL_LAST_REFIT, info
    got = tr.query_rays(qu.as_rows(rays))
    assert not (got["renderNode"] == hide).any() and (before["renderNode"] == hide).any()
    assert not (tr.query_rays(qu.as_rows(rays), mode="any")["renderNode"] == hide).any()
    assert got.tobytes() == _fresh_bytes(st.scene, rays).tobytes()
    # a material-id change (a variant switch): the records' materialID follows, by a patch
    patches = tr.accel_resident_info()["materialPatches"]
    assert st.scene.set_variant(1) > 0
    tr.update_render_nodes(d.renderNodes, d.numRenderNodes, d.renderNodeVisible)
    assert tr.accel_resident_info()["materialPatches"] == patches + 1
    switched = tr.query_rays(qu.as_rows(rays))
    assert switched.tobytes() == _fresh_bytes(st.scene, rays).tobytes()
    h = switched["renderNode"] >= 0
    want = np.array([max(0, d.renderNodes[int(n)].materialID) for n in switched["renderNode"][h]])
    assert (switched["materialID"][h] == want).all()
    assert (switched["materialID"] != got["materialID"]).any()
    other = [n for n in switched.dtype.names if n != "materialID"]
    assert all((switched[n] == got[n]).all() for n in other)  # nothing but the material changed
    tr.close()


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------------------
def _holder(desc, keep):
    class Holder:
        pass
    h = Holder()
    h.desc = C.pointer(desc)
    h._keep = keep
    return h


def _copy_desc(scene):
    d = scene.desc.contents
    desc = type(d)()
    C.memmove(C.byref(desc), C.byref(d), C.sizeof(desc))
    return desc


@pytest.mark.parametrize("bvh", [0, 1])
def test_empty_and_one_triangle_scenes(animated, bvh):
    scene = ptmod.Scene(animated)
    st, rays = _rays_for(scene, n=300)
    # nothing visible: every ray misses, in both modes
    desc = _copy_desc(scene)
    hidden = (C.c_uint8 * desc.numRenderNodes)()
    desc.renderNodeVisible = C.cast(hidden, C.POINTER(C.c_uint8))
    tr = ptmod.PathTracer(_holder(desc, [hidden]), bvh=bvh)
    assert tr.stats()["bvhTriangleCount"] == 0
    for mode in ("closest", "any"):
        m = tr.query_rays(qu.as_rows(rays), mode=mode)
        assert (m["renderNode"] == -1).all() and (m["flags"] == 0).all() and not m["position"].any()
    tr.close()
    # one triangle: render node 0 alone, its primitive cut down to its first triangle
    desc = _copy_desc(scene)
    node = (capi.MiGltfRenderNode * 1)()
    C.memmove(node, desc.renderNodes, C.sizeof(node))
    prims = (capi.MiPtRenderPrimitive * desc.numRenderPrimitives)()
    C.memmove(prims, desc.renderPrimitives, C.sizeof(prims))
    prims[node[0].renderPrimID].triangleCount = 1
    prims[node[0].renderPrimID].opaqueTriangleCount = 0
    desc.renderNodes, desc.numRenderNodes, desc.renderNodeVisible, desc.renderPrimitives = node, 1, None, prims
    holder = _holder(desc, [node, prims])
    tr = ptmod.PathTracer(holder, bvh=bvh)
    assert tr.stats()["bvhTriangleCount"] == 1
    one = qu.SceneTris(holder)
    assert len(one) == 1
    # rays at the triangle from both sides, and rays past it
    c = one.V[0].mean(0)
    n = np.cross(one.e1[0], one.e2[0])
    n /= np.linalg.norm(n)
    aim = qu.make_rays(st, n=8, seed=3)
    for k in range(8):
        side = 1.0 if k % 2 == 0 else -1.0
        o = c + side * (1.0 + k) * n + 0.01 * k * one.e1[0]
        aim["origin"][k] = o
        aim["direction"][k] = (c - o) / np.linalg.norm(c - o)
    batch = np.concatenate([aim, rays])
    ref = qu.Reference(qu.Pairs(one, batch))
    got = tr.query_rays(qu.as_rows(batch))
    assert ((got["flags"][:8] & HIT) != 0).all() and ((got["flags"][:8:2] & FRONT) != 0).all() and ((got["flags"][1:8:2] & FRONT) == 0).all()
    qu.check_hits(one, batch, ref, got, *qu.TOLERANCE["animated"], what="one triangle, bvh %d" % bvh)
    anyhit = tr.query_rays(qu.as_rows(batch), mode="any")
    assert anyhit.tobytes() == got.tobytes()  # one triangle: the first accepted is the closest
    tr.close()
    scene.close()


def test_batch_sizes_and_invalid_rays(cases):
    c = cases("animated")
    rows = qu.as_rows(c.rays)
    assert len(c.wide.query_rays(rows[:0])) == 0
    for tr, whole in ((c.wide, c.closest), (c.bvh2, c.closest2)):
        for n in (1, 63, 64, 65, 257):
            part = tr.query_rays(rows[:n])
            assert part.tobytes() == whole[:n].tobytes(), n
            tail = tr.query_rays(rows[-n:], mode="any")
            assert (((tail["flags"] & HIT) != 0) == ((whole[-n:]["flags"] & HIT) != 0)).all(), n
        # invalid rays among valid ones: their own records say so, the neighbours are undisturbed
        mixed = rows[:257].copy()
        bad = {3: (0, np.nan), 64: (4, np.inf), 65: (5, -np.inf), 130: (3, np.nan), 200: (7, np.nan), 256: (2, np.inf)}
        for i, (col, val) in bad.items():
            mixed[i, col] = val
        mixed[10, 4:7] = 0.0  # a zero direction
        bad[10] = None
        for mode in ("closest", "any"):
            got = tr.query_rays(mixed, mode=mode)
            idx = np.array(sorted(bad))
            assert (got["flags"][idx] == INVALID).all() and (got["renderNode"][idx] == -1).all()
            z = got[idx].copy()
            z["flags"], z["renderNode"] = 0, 0
            assert not z.view(np.uint8).any()
            good = np.setdiff1d(np.arange(257), idx)
            if mode == "closest":
                assert got[good].tobytes() == whole[:257][good].tobytes()
            else:
                assert (((got["flags"][good] & HIT) != 0) == ((whole[:257]["flags"][good] & HIT) != 0)).all()
    with pytest.raises(ptmod.MiError):
        c.wide.query_rays(rows[:4], mode=2)
    assert c.wide._l.mi_pt_query_rays(c.wide._p, None, 4, 0, None) == -1  # MI_PT_ERR_ARGUMENT: NULL pointers with a positive count
    assert c.wide._l.mi_pt_query_rays(c.wide._p, None, -1, 0, None) == -1
    assert c.wide._l.mi_pt_query_rays_device(c.wide._p, None, 4, 0, None, None) == -1
    assert c.wide._l.mi_pt_query_rays_device(c.wide._p, None, 0, 0, None, None) == 0
    assert c.wide._l.mi_pt_pick(c.wide._p, None, 4, None) == -1
    assert c.wide._l.mi_pt_query_rays(c.wide._p, None, 0, 0, None) == 0


# ---- 6. the device form ---------------------------------------------------------------------------------------------------------------------------
def test_device_form_with_torch_tensors(tmp_path):
    """In a process of its own (tests/query_device_child.py): torch brings its own copy of the HIP runtime, and the two libraries share one only
    when torch is loaded first -- which no test of a long pytest process can arrange.  The child checks that a torch tensor goes in and the records
    equal the host form's byte for byte in both trees, that a query between queued frames leaves the accumulator bit-identical, and that the
    device form allocates nothing."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "query_device_child.py"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "QUERY_DEVICE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---- 7. side effects ------------------------------------------------------------------------------------------------------------------------------
def test_memory_and_counters(animated):
    st = pu.Setup(animated, W, H, max_depth=3)
    _, rays = _rays_for(st.scene, n=1000)
    rows = qu.as_rows(rays)
    tr = _tracer(st, collect_counters=True)
    tr.enable_timing(True)
    _render(tr, st, frames=2)
    m0, s0, t0 = tr.memory(), tr.stats(), tr.frame_timing()
    keys = ("sceneBytes", "rendererBytes", "pathStateBytes", "pathSlots")
    # the host forms stage: 32 + 64 bytes per ray from the first call on, grown, never shrunk -- so there was nothing before it
    tr.query_rays(rows[:300])
    m1 = tr.memory()
    assert m1["rendererBytes"] - m0["rendererBytes"] == 300 * (32 + 64) and all(m1[k] == m0[k] for k in keys if k != "rendererBytes")
    tr.query_rays(rows[:100], mode="any")
    tr.pick(_centres()[:200])
    assert tr.memory()["rendererBytes"] == m1["rendererBytes"]
    tr.pick(_centres()[:1000])
    tr.query_rays(rows)
    assert tr.memory()["rendererBytes"] - m0["rendererBytes"] == 1000 * (32 + 64)
    assert tr.stats() == s0
    t1 = tr.frame_timing()
    assert t1 == t0, (t0, t1)
    tr.close()
