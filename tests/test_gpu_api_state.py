"""The C-ABI's host-side state (csrc/device/mi_pt_api.hip), pinned from outside: the whole-image read-backs against an independent route to
the same memory, the slot-to-pixel scatter under a tile partition, what each feature allocates and releases (mi_pt_get_memory round trips),
the update counters, and the three denoise calls with and without a host destination.

One instance over assets/Box.glb at 40 x 24 with 16-pixel tiles: not square, no multiple of the tile size in either direction, 3 x 2 tiles
of which four are cut by the image border.  One frame per render."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as pu
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, TILE = 40, 24, 16
PX = W * H
GUARD = 0xA5C3F00D


class Box:
    pass


@pytest.fixture(scope="module")
def box():
    b = Box()
    b.st = pu.Setup(os.path.join(ROOT, "assets", "Box.glb"), W, H, max_depth=3)
    b.tr = ptmod.PathTracer(b.st.scene)
    b.tr.set_tile_partition(0, 1, TILE)
    b.tr.resize(W, H)
    b.tr.set_frame_info(b.st.frame_info)
    b.tr.set_sky(b.st.sky)
    d = b.st.scene.desc.contents
    b.prim = next(i for i in range(int(d.numRenderPrimitives)) if d.renderPrimitives[i].triangleCount > 0 and d.renderPrimitives[i].normals)
    b.vertices, b.triangles = int(d.renderPrimitives[b.prim].vertexCount), int(d.renderPrimitives[b.prim].triangleCount)
    b.nodes, b.textures = int(d.numRenderNodes), int(d.numTextures)
    yield b
    b.tr.close()


def _first_frame(b, guides=False):
    p = b.st.frame_params(0, 0)
    if guides:
        p.flags |= capi.MI_PT_USE_OPTIX_DENOISER
    b.tr.render_frame(p)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _same(a, b):
    return np.array_equal(_bytes(a), _bytes(b))


def _totals(tr):
    m = tr.memory()
    return m["sceneBytes"], m["rendererBytes"]


# ---- 1. read-backs against an independent route ------------------------------------------------------------------------------------------------
def test_read_backs_equal_the_bound_tensors():
    """In a process of its own (tests/api_state_device_child.py): torch brings its own copy of the HIP runtime, and the two libraries share one
    only when torch is loaded first.  The child binds the accumulator and the three guide images to torch tensors, renders one first frame
    with the guides on and checks that mi_pt_read_accum, mi_pt_read_guides (each image alone and both together) and mi_pt_read_depth equal
    the tensors byte for byte; unbound, that mi_pt_read_accum equals the memory behind mi_pt_accum_device_ptr."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "api_state_device_child.py")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "API_STATE_DEVICE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_selection_and_motion_fill_the_image_and_nothing_behind_it(box):
    tr, lib = box.tr, box.tr._l
    tr.set_temporal(True)
    try:
        _first_frame(box)
        sel = np.full(PX + 1, GUARD, np.uint32)
        assert lib.mi_pt_read_selection(tr._p, sel.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
        assert sel[PX] == GUARD and (sel[:PX] != GUARD).all()
        assert _same(sel[:PX], tr.read_selection())
        mot = np.full(PX * 4 + 4, GUARD, np.uint32)
        assert lib.mi_pt_read_motion(tr._p, mot.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))) == 0
        assert (mot[PX * 4:] == GUARD).all() and (mot[:PX * 4].reshape(PX, 4) != GUARD).any(axis=1).all()
        assert _same(mot[:PX * 4], tr.read_motion()) and tr.read_motion().nbytes == PX * 16 and tr.read_selection().nbytes == PX * 4
    finally:
        tr.set_temporal(False)


# ---- 2. the scatter -----------------------------------------------------------------------------------------------------------------------------
def test_scatter_under_a_tile_partition(box):
    tr = box.tr
    tr.set_temporal(True)
    tr.set_vertex_updates([box.prim])
    tr.set_vertex_motion(True)
    try:
        _first_frame(box)
        hit_all, tri_all = tr.read_first_hit(), tr.read_first_hit_triangle()
        assert (hit_all.view(np.uint32)[..., 3] != 0).any() and (tri_all[..., 0] != 0xffffffff).any()
        tiles_x = (W + TILE - 1) // TILE
        tile_of = (np.arange(H)[:, None] // TILE) * tiles_x + np.arange(W)[None, :] // TILE  # (tile t belongs to rank t % world)
        for rank in (0, 1):
            tr.set_tile_partition(rank, 2, TILE)
            _first_frame(box)
            owned = (tile_of % 2) == rank
            assert owned.any() and (~owned).any()
            hit, tri = tr.read_first_hit(), tr.read_first_hit_triangle()
            assert (_bytes(hit).reshape(H, W, 16)[~owned] == 0).all()
            assert (_bytes(tri).reshape(H, W, 16)[~owned] == 0xff).all()
            assert _same(hit[owned], hit_all[owned]) and _same(tri[owned], tri_all[owned])
    finally:
        tr.set_tile_partition(0, 1, TILE)
        tr.set_vertex_motion(False)
        tr.set_vertex_updates(None)
        tr.set_temporal(False)


# ---- 3. groups release everything and only themselves -------------------------------------------------------------------------------------------
def _one_joint_skin(b):
    """The smallest skin there is: the box's primitive bound to one joint with full weight (the deformation tests' scenes are other scenes;
    this one deforms the instance under test)."""
    pos, nrm, _ = b.tr.read_vertices(b.prim)
    joints = np.zeros((b.vertices, 4), np.uint16)
    weights = np.zeros((b.vertices, 4), np.float32)
    weights[:, 0] = 1.0
    p = capi.MiPtDeformPrimitive()
    p.renderPrimID, p.vertexCount = b.prim, b.vertices
    p.basePositions = pos.ctypes.data_as(C.POINTER(C.c_float))
    p.baseNormals = nrm.ctypes.data_as(C.POINTER(C.c_float))
    p.joints = joints.ctypes.data_as(C.POINTER(C.c_uint16))
    p.weights = weights.ctypes.data_as(C.POINTER(C.c_float))
    p.numJoints = 1
    table = (capi.MiPtDeformPrimitive * 1)(p)
    d = capi.MiPtDeformDesc()
    d.prims, d.numPrims, d.numJointMatrices = table, 1, 1
    return d, (pos, nrm, joints, weights, table)


def test_groups_release_everything_and_only_themselves(box):
    tr, lib = box.tr, box.tr._l
    start = _totals(tr)
    assert tr.vertex_update_info()["tableBytes"] == 0 and tr.accel_info()["refitBytes"] == 0

    # vertex updates: the incident-corner tables (V run ends + 3 T corners, 4 bytes each) and the three task buffers, all sceneBytes.  The task
    # records' sizes are not part of the binding: the rise is bounded from below (the block table alone holds 2 blocks + 1 words)
    tr.set_vertex_updates([box.prim], recompute_normals=True)
    table = tr.vertex_update_info()["tableBytes"]
    assert table == 4 * (box.vertices + 3 * box.triangles)
    scene, renderer = _totals(tr)
    assert scene > start[0] + table + 12 and renderer == start[1]
    tr.set_vertex_updates([])
    assert _totals(tr) == start and tr.vertex_update_info()["tableBytes"] == 0

    # deformation tables
    desc, keep = _one_joint_skin(box)
    assert lib.mi_pt_set_deformation(tr._p, C.byref(desc)) == 0
    scene, renderer = _totals(tr)
    # (the pool: 48 B base pose + 8 B joints + 16 B weights per vertex; the joint table: 6 float4; one morph weight slot)
    assert scene >= start[0] + box.vertices * 72 + 96 + 4 and renderer == start[1]
    assert lib.mi_pt_set_deformation(tr._p, None) == 0
    assert _totals(tr) == start
    del keep

    # temporal: motion image, two history sets of three records, the previous matrices -- all rendererBytes
    tr.set_temporal(True)
    assert _totals(tr) == (start[0], start[1] + PX * 16 + 6 * PX * 16 + box.nodes * 64)
    tr.set_temporal(False)
    assert _totals(tr) == start

    # vertex motion while temporal and vertex updates are on: the previous positions (12 B per vertex, padded to 16), one record per render
    # primitive and the id list in sceneBytes, the first-hit triangle records (one uint4 per pixel slot) in rendererBytes
    tr.set_temporal(True)
    tr.set_vertex_updates([box.prim])
    before = _totals(tr)
    tr.set_vertex_motion(True)
    scene, renderer = _totals(tr)
    slots = tr.memory()["pathSlots"]
    assert slots == 6 * TILE * TILE
    assert scene >= before[0] + ((box.vertices * 12 + 15) & ~15) + 4 and renderer == before[1] + slots * 16
    tr.set_vertex_motion(False)
    assert _totals(tr) == before
    tr.set_vertex_motion(True)   # in force again, then released by each of the other two switches
    tr.set_vertex_updates([])
    tr.set_temporal(False)
    tr.set_vertex_motion(False)
    assert _totals(tr) == start

    # refit data
    tr.set_accel_update("refit")
    info = tr.accel_info()
    assert info["refitBytes"] > 0 and info["sahCostAtBuild"] > 0
    assert _totals(tr) == (start[0] + info["refitBytes"], start[1])
    tr.set_accel_update("rebuild")
    info = tr.accel_info()
    assert info["refitBytes"] == 0 and info["sahCostAtBuild"] == 0 and info["sahCost"] == 0
    assert _totals(tr) == start

    _first_frame(box)
    assert np.isfinite(tr.read_accum()).all()


# ---- 4. counters ------------------------------------------------------------------------------------------------------------------------------
def test_counters_survive_what_they_survived_before(box):
    tr, lib = box.tr, box.tr._l
    v0, t0, e0 = tr.vertex_update_info()["calls"], tr.texture_update_info()["calls"], tr.environment_update_info()["calls"]
    pos, _, _ = tr.read_vertices(box.prim)
    tr.set_vertex_updates([box.prim])
    tr.update_vertices({box.prim: pos})
    tr.update_vertices({box.prim: pos})
    info = tr.vertex_update_info()
    assert info["calls"] == v0 + 2 and info["verticesRejected"] == 0
    written = info["verticesWritten"]
    tr.set_vertex_updates([])
    tr.set_vertex_updates([box.prim])
    assert tr.vertex_update_info()["calls"] == v0 + 2 and tr.vertex_update_info()["verticesWritten"] == written
    tr.set_vertex_updates([])

    if box.textures > 0:
        t = box.st.scene.desc.contents.textures[0]
        img = np.full((int(t.height), int(t.width), 4), 128, np.uint8)
        tr.update_textures({0: img})
        tr.update_textures({0: img})
    else:  # (the box has no texture: a call that brings no update is a call all the same)
        assert lib.mi_pt_update_textures(tr._p, None, 0) == 0 and lib.mi_pt_update_textures(tr._p, None, 0) == 0
    assert tr.texture_update_info()["calls"] == t0 + 2

    env = np.full((2, 4, 3), 0.5, np.float32)
    tr.update_environment(env)
    tr.update_environment(env)
    info = tr.environment_update_info()
    assert info["calls"] == e0 + 2 and info["texelsWritten"] >= 16 and info["scratchBytes"] > 0 and info["integral"] > 0
    assert info["lightTexels"] + info["heavyTexels"] == 8


# ---- 5. denoise paths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["atrous", "svgf", "temporal"])
def test_denoise_with_and_without_a_host_destination(box, which):
    tr, lib = box.tr, box.tr._l
    tp = tr.default_temporal()

    def call(host):
        dst = host.ctypes.data_as(C.POINTER(C.c_float)) if host is not None else None
        if which == "atrous":
            return lib.mi_pt_denoise(tr._p, 3, 0.6, 64.0, 0.2, dst, None)
        if which == "svgf":
            return lib.mi_pt_denoise_svgf(tr._p, 3, 4.0, 128.0, 1.0, dst, None)
        return lib.mi_pt_denoise_temporal(tr._p, C.byref(tp), dst, None)

    if which == "temporal":
        tr.set_temporal(True)
    try:
        _first_frame(box, guides=True)
        out = np.full(PX * 4 + 4, np.nan, np.float32)
        assert call(out) == 0
        assert np.isfinite(out[:PX * 4]).all() and np.isnan(out[PX * 4:]).all()
        renderer = tr.memory()["rendererBytes"]
        assert call(None) == 0
        tr.synchronize()
        assert lib.mi_pt_denoised_device_ptr(tr._p)
        again = np.full(PX * 4, np.nan, np.float32)
        assert call(again) == 0 and np.isfinite(again).all()
        assert tr.memory()["rendererBytes"] == renderer
    finally:
        if which == "temporal":
            tr.set_temporal(False)
