"""CPU tier of vertex motion (mi_pt_set_vertex_motion): csrc/device/pt_temporal.h's motionRecordDeformed compiled for the host through
tests/host_shim (g++ -ffp-contract=off) and diffed against the float64 restatement of tests/vertex_motion_util.py, which is written from
the definition (previous world position = prevObjectToWorld x barycentric sum of the previous-pose vertices); the rigid path and the
fallbacks byte for byte against motionRecord; and the public surface: the three entry points in the header, the binding and the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_util as tu
import vertex_motion_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U, P = C.c_float, C.c_uint32, C.POINTER
ENTRY_POINTS = ("mi_pt_set_vertex_motion", "mi_pt_read_first_hit_triangle", "mi_pt_read_previous_positions")
N_SURFACE, N_SKY = 1600, 400
N = N_SURFACE + N_SKY


class ShimPrim(C.Structure):
    _fields_ = [("prevPositions", P(F)), ("positions", P(F)), ("indices", P(U)), ("numTriangles", U), ("vertexCount", U)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vertex_motion_shim") / "libvertex_motion_on_host.so")
    d = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-I" + d, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"), "-o", out, os.path.join(d, "vertex_motion_on_host.cpp")], check=True)
    L = C.CDLL(out)
    L.dev_vertex_motion_records.argtypes = [C.c_int, P(F), P(U), P(ShimPrim), C.c_int, C.c_void_p, P(F), C.c_int, P(F), P(F), F, F, P(F)]
    L.dev_vertex_motion_records.restype = None
    L.dev_rigid_motion_records.argtypes = [C.c_int, P(F), C.c_void_p, P(F), C.c_int, P(F), P(F), F, F, P(F)]
    L.dev_rigid_motion_records.restype = None
    return L


def fp(a):
    return a.ctypes.data_as(P(F))


def _rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _rigid(rng, max_angle, max_shift):
    M = np.eye(4)
    M[:3, :3] = _rotation(rng.normal(size=3), rng.uniform(-max_angle, max_angle))
    M[:3, 3] = rng.uniform(-max_shift, max_shift, 3)
    return M


def _view_proj(eye, yaw, pitch, fov_deg, aspect, near=0.1, far=1000.0):
    R = _rotation(np.array([1.0, 0, 0]), pitch) @ _rotation(np.array([0, 1.0, 0]), yaw)
    V = np.eye(4)
    V[:3, :3] = R
    V[:3, 3] = -R @ eye
    f = 1.0 / np.tan(np.radians(fov_deg) / 2)
    Pm = np.array([[f / aspect, 0, 0, 0], [0, -f, 0, 0], [0, 0, far / (near - far), near * far / (near - far)], [0, 0, -1, 0]])
    return Pm @ V


def _cm(M):
    return np.ascontiguousarray(M.T, np.float32).reshape(16)


def _case(seed):
    """1 600 surface hits on 8 render nodes (3 of which stand still) and 400 sky directions under two cameras, as the rigid tier's case;
    every surface hit lies on a triangle of its own whose barycentric sum of the CURRENT vertices is the hit in object space.  Three render
    primitives: 0 and 2 deform (previous positions = current + a displacement of up to 0.2 per axis), 1 does not.  The first 120 hits carry
    the vertex and edge barycentrics.  Points at 4 .. 40 units from cameras near the origin: both clip w stay >= 0.1."""
    rng = np.random.default_rng(seed)
    W, H = 1920.0, 1080.0
    eye, yaw, pitch = rng.uniform(-1, 1, 3), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)
    vp = _view_proj(eye, yaw, pitch, 45.0, W / H)
    pm = _view_proj(eye + rng.uniform(-0.2, 0.2, 3), yaw + np.radians(2.0), pitch - np.radians(1.0), 45.0, W / H)
    K = 8
    cur = [_rigid(rng, 0.8, 0.5) for _ in range(K)]
    prev = [c if k < 3 else _rigid(rng, np.radians(5.0), 0.3) @ c for k, c in enumerate(cur)]
    o2w, w2o, pv = np.stack([_cm(c) for c in cur]), np.stack([_cm(np.linalg.inv(c)) for c in cur]), np.stack([_cm(c) for c in prev])
    ndc = rng.uniform(-0.8, 0.8, (N, 2))
    far_pt = (np.linalg.inv(vp) @ np.concatenate([ndc, np.full((N, 1), 0.5), np.ones((N, 1))], 1).T).T
    d = far_pt[:, :3] / far_pt[:, 3:4] - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    fh = np.zeros((N, 4), np.float32)
    fh[:N_SURFACE, :3] = eye + d[:N_SURFACE] * rng.uniform(4.0, 40.0, N_SURFACE)[:, None]
    fh[N_SURFACE:, :3] = d[N_SURFACE:]
    ids = np.zeros(N, np.uint32)
    ids[:N_SURFACE] = rng.integers(1, K + 1, N_SURFACE)
    fh[:, 3] = ids.view(np.float32)
    # barycentrics: vertices, edges (b1 = 0, b2 = 0, b1 + b2 = 1), then the interior
    b1 = rng.uniform(0.0, 1.0, N).astype(np.float32)
    b2 = (rng.uniform(0.0, 1.0, N) * (1.0 - b1)).astype(np.float32)
    b1[0:20], b2[0:20] = 0.0, 0.0
    b1[20:40], b2[20:40] = 1.0, 0.0
    b1[40:60], b2[40:60] = 0.0, 1.0
    b1[60:80] = 0.0
    b2[80:100] = 0.0
    b2[100:120] = np.float32(1.0) - b1[100:120]
    prim_of = rng.integers(0, 3, N).astype(np.uint32)
    prim_of[:120] = np.where(prim_of[:120] == 1, 0, prim_of[:120])  # (the special barycentrics all on deforming primitives)
    tri = np.zeros((N, 4), np.uint32)
    tri[:, 0], tri[:, 2], tri[:, 3] = prim_of, b1.view(np.uint32), b2.view(np.uint32)
    prims = {}
    for pid in range(3):
        hits = np.nonzero(prim_of == pid)[0]
        tri[hits, 1] = np.arange(len(hits))
        verts = rng.uniform(-0.5, 0.5, (len(hits), 3, 3))
        b = np.stack([1.0 - b1[hits].astype(np.float64) - b2[hits], b1[hits], b2[hits]], 1)
        for j, i in enumerate(hits):
            target = (np.linalg.inv(cur[ids[i] - 1]) @ np.append(fh[i, :3].astype(np.float64), 1.0))[:3] if ids[i] else np.zeros(3)
            verts[j] += target - b[j] @ verts[j]
        cur_pos = verts.reshape(-1, 3).astype(np.float32)
        prev_pos = (cur_pos + rng.uniform(-0.2, 0.2, cur_pos.shape)).astype(np.float32) if pid != 1 else None
        prims[pid] = dict(indices=np.arange(3 * len(hits), dtype=np.uint32).reshape(-1, 3), cur=cur_pos, prev=prev_pos)
    return dict(fh=fh, tri=tri, prims=prims, o2w=o2w, w2o=w2o, pv=pv, vp=_cm(vp), pm=_cm(pm), W=W, H=H)


def _nodes(c):
    nodes = np.zeros((len(c["o2w"]), 34), np.float32)  # MiGltfRenderNode: objectToWorld, worldToObject, materialID, renderPrimID
    nodes[:, :16], nodes[:, 16:32] = c["o2w"], c["w2o"]
    return nodes


def _run(shim, c, fh=None, tri=None, prims=None, pv=None, pm=None, num_prims=None):
    fh = np.ascontiguousarray(c["fh"] if fh is None else fh, np.float32)
    tri = np.ascontiguousarray(c["tri"] if tri is None else tri, np.uint32)
    prims = c["prims"] if prims is None else prims
    pv = np.ascontiguousarray(c["pv"] if pv is None else pv, np.float32)
    pm = c["pm"] if pm is None else pm
    count = len(prims) if num_prims is None else num_prims
    table = (ShimPrim * len(prims))()
    keep = []
    for pid, p in prims.items():
        arrays = [None if p["prev"] is None else np.ascontiguousarray(p["prev"], np.float32), np.ascontiguousarray(p["cur"], np.float32),
                  np.ascontiguousarray(p["indices"], np.uint32)]
        keep.append(arrays)
        table[pid].prevPositions = None if arrays[0] is None else fp(arrays[0])
        table[pid].positions = fp(arrays[1])
        table[pid].indices = arrays[2].ctypes.data_as(P(U))
        table[pid].numTriangles, table[pid].vertexCount = len(arrays[2]), len(arrays[1])
    nodes = _nodes(c)
    got, rigid = np.zeros((len(fh), 4), np.float32), np.zeros((len(fh), 4), np.float32)
    shim.dev_vertex_motion_records(len(fh), fp(fh), tri.ctypes.data_as(P(U)), table, count, nodes.ctypes.data_as(C.c_void_p), fp(pv), len(nodes), fp(c["vp"]),
                                   fp(pm), c["W"], c["H"], fp(got))
    shim.dev_rigid_motion_records(len(fh), fp(fh), nodes.ctypes.data_as(C.c_void_p), fp(pv), len(nodes), fp(c["vp"]), fp(pm), c["W"], c["H"], fp(rigid))
    return got, rigid


# ---- random data against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [20261017, 7])
def test_deformed_motion_matches_the_float64_definition(shim, seed):
    c = _case(seed)
    got, rigid = _run(shim, c)
    want, clipw, deformed = vu.vertex_motion_numpy(c["fh"], c["tri"], c["prims"], c["o2w"], c["w2o"], c["pv"], c["vp"], c["pm"], c["W"], c["H"])
    assert (np.abs(clipw) >= 0.1).all(), "the generator left a point outside the stated condition (both clip w >= 0.1)"
    on_deforming = c["tri"][:N_SURFACE, 0] != 1
    assert np.array_equal(deformed[:N_SURFACE], on_deforming) and not deformed[N_SURFACE:].any() and deformed[:120].all()
    err = np.abs(got[:, :2] - want[:, :2])
    print("motion |delta| px: max %.3g, deformed %.3g, edge / vertex barycentrics %.3g, rigid %.3g, sky %.3g" % (
        err.max(), err[deformed].max(), err[:120].max(), err[:N_SURFACE][~on_deforming].max(), err[N_SURFACE:].max()))
    # the bounds of the rigid tier (test_motion_vector_matches_the_reference_definition): the chain has the same length -- the barycentric
    # sum stands where the worldToObject product stood, then the previous objectToWorld and the projection
    assert err.max() <= 1e-3
    assert np.abs(got[:N_SURFACE, 2] - want[:N_SURFACE, 2]).max() <= 1e-6 and (got[N_SURFACE:, 2] == 1.0).all()
    assert np.array_equal(got[:, 3].view(np.uint32), c["fh"][:, 3].view(np.uint32))
    # the case really deforms: the deformed hits are far from where the rigid record puts them, the others ARE the rigid record
    assert np.abs(got[deformed, :2] - rigid[deformed, :2]).max() > 10.0
    assert np.array_equal(got[~deformed].view(np.uint32), rigid[~deformed].view(np.uint32))


# ---- the rigid path, bit for bit -----------------------------------------------------------------------------------------------------
def _still(prims):
    return {pid: dict(p, prev=None if p["prev"] is None else p["cur"].copy()) for pid, p in prims.items()}


def test_equal_previous_positions_give_the_rigid_record(shim):
    c = _case(11)
    got, rigid = _run(shim, c, prims=_still(c["prims"]))  # moved nodes, two cameras, previous == current positions bit for bit
    assert np.array_equal(got.view(np.uint32), rigid.view(np.uint32))
    assert np.abs(rigid[:N_SURFACE, :2]).max() > 10.0
    # one differing bit in one coordinate of one vertex takes that triangle, and no other, off the rigid path
    prims = _still(c["prims"])
    hit = int(np.nonzero((c["tri"][:, 0] == 0) & (c["tri"][:, 1] == 5))[0][0])
    prims[0]["prev"].view(np.uint32)[3 * 5 + 1, 2] ^= 1
    got2, _ = _run(shim, c, prims=prims)
    others = np.arange(N) != hit
    assert np.array_equal(got2[others].view(np.uint32), rigid[others].view(np.uint32))
    # nothing moved at all: exactly zero, not merely small
    got, _ = _run(shim, c, prims=_still(c["prims"]), pv=c["o2w"], pm=c["vp"])
    assert (got[:, :2] == 0.0).all()


# ---- fallbacks -----------------------------------------------------------------------------------------------------------------------
def test_records_without_a_deforming_triangle_fall_back_to_the_rigid_record(shim):
    c = _case(5)
    fh, tri = c["fh"][:8].copy(), c["tri"][:8].copy()
    assert (tri[:, 0] != 1).all() and (fh[:, 3].view(np.uint32) != 0).all()
    ids = fh[:, 3].view(np.uint32)
    ids[0] = 0                      # id 0: a direction, whatever the triangle record says
    ids[1] = 0xFFFFFFFF             # the invalid id
    tri[2, 0] = vu.NO_PRIM          # no primitive
    tri[3, 0] = 1                   # a primitive without previous positions
    tri[4, 0] = 3                   # a primitive beyond the table
    tri[5, 1] = 1 << 30             # a triangle beyond the primitive
    ids[6] = len(c["o2w"]) + 1      # a render node beyond the table
    got, rigid = _run(shim, c, fh=fh, tri=tri)
    assert np.array_equal(got[:7].view(np.uint32), rigid[:7].view(np.uint32))
    assert not np.array_equal(got[7].view(np.uint32), rigid[7].view(np.uint32))  # (the untouched record does take the deformed path)
    assert (got[1, :2] == 0.0).all() and got[1, 3:].view(np.uint32)[0] == 0xFFFFFFFF and got[6, 3:].view(np.uint32)[0] == 0xFFFFFFFF
    # a table of no primitives at all
    got, rigid = _run(shim, c, num_prims=0)
    assert np.array_equal(got.view(np.uint32), rigid.view(np.uint32))


# ---- public surface ------------------------------------------------------------------------------------------------------------------
def test_vertex_motion_entry_points_are_declared_bound_and_exported(built):
    from vk_gltf_renderer_amd import _capi as capi
    header = open(os.path.join(ROOT, "include", "mi_pt.h")).read()
    assert re.search(r"#define MI_PT_ABI_VERSION 9\b", header)
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vk_gltf_renderer_amd", "lib", "libmi_pt.so")], check=True,
                              capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(r"MI_PT_API\s+\w+\s+%s\(" % name, header), name
        assert name in capi.PT_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    assert capi.MI_PT_ABI_VERSION == 9 and capi.pt_lib().mi_pt_abi_version() == 9
    from vk_gltf_renderer_amd import pathtracer as ptmod
    for name in ("set_vertex_motion", "read_first_hit_triangle", "read_previous_positions"):
        assert callable(getattr(ptmod.PathTracer, name))
