"""CPU tier of caller-driven vertex updates (mi_pt_set_vertex_updates / mi_pt_update_vertices): the per-vertex functions of
csrc/device/pt_vertex_update.h compiled for the host through tests/host_shim (g++ -ffp-contract=off).  What they write is compared byte
for byte with the interleaving loop of mi_pt_create restated in numpy (tests/vertex_update_util.py), the rejection rule is checked on arrays
salted with NaN and +-inf, the normal rebuild against a float64 restatement written from its definition; and the public surface: the
entry points in the header, the binding and the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vertex_update_util as vu
from vk_gltf_renderer_amd import scenegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U, B, P = C.c_float, C.c_uint32, C.c_uint8, C.POINTER
ENTRY_POINTS = ("mi_pt_set_vertex_updates", "mi_pt_update_vertices", "mi_pt_update_vertices_device", "mi_pt_get_vertex_update_info")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vertex_update_shim") / "libvertex_update_on_host.so")
    d = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-I" + d, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"), "-o", out, os.path.join(d, "vertex_update_on_host.cpp")], check=True)
    L = C.CDLL(out)
    L.dev_vertex_ingest.argtypes = [U, P(F), P(F), P(F), P(F), P(F), P(F), P(F), P(B)]
    L.dev_vertex_ingest.restype = U
    L.dev_rebuild_normals.argtypes = [U, P(F), P(U), P(U), P(U), P(F), P(F)]
    L.dev_rebuild_normals.restype = None
    return L


def fp(a):
    return None if a is None else a.ctypes.data_as(P(F))


class Resident:
    """The streams and the interleaved record of one primitive as mi_pt_create leaves them."""

    def __init__(self, rng, nv, normals, uv0, tangents):
        self.pos = rng.uniform(-2, 2, (nv, 3)).astype(np.float32)
        self.nrm = rng.normal(size=(nv, 3)).astype(np.float32) if normals else None
        self.uv0 = rng.uniform(0, 1, (nv, 2)).astype(np.float32) if uv0 else None
        self.tan = rng.normal(size=(nv, 4)).astype(np.float32) if tangents else None
        self.verts = vu.interleave(self.pos, self.nrm, self.uv0, self.tan)

    def ingest(self, shim, pos, nrm=None, tan=None):
        rejected = np.zeros(len(self.pos), np.uint8)
        n = shim.dev_vertex_ingest(len(self.pos), fp(pos), fp(nrm), fp(tan), fp(self.pos), fp(self.nrm), fp(self.tan), fp(self.verts),
                                   rejected.ctypes.data_as(P(B)))
        return n, rejected.astype(bool)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- a vertex write is what mi_pt_create would upload ------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals,uv0,tangents", [(True, True, True), (True, False, False), (False, False, False), (True, True, False), (False, True, False)])
@pytest.mark.parametrize("nv", [1, 3, 336])
def test_written_records_are_the_interleaving_of_mi_pt_create(shim, nv, normals, uv0, tangents):
    rng = np.random.default_rng(nv * 8 + normals * 4 + uv0 * 2 + tangents)
    r = Resident(rng, nv, normals, uv0, tangents)
    pos = rng.uniform(-3, 3, (nv, 3)).astype(np.float32)
    nrm = rng.normal(size=(nv, 3)).astype(np.float32) if normals else None
    tan = rng.normal(size=(nv, 4)).astype(np.float32) if tangents else None
    n, rejected = r.ingest(shim, pos, nrm, tan)
    assert n == 0 and not rejected.any()
    assert same(r.pos, pos) and (nrm is None or same(r.nrm, nrm)) and (tan is None or same(r.tan, tan))
    assert same(r.verts, vu.interleave(pos, nrm, r.uv0, tan))


def test_a_stream_that_is_not_supplied_keeps_its_bytes(shim):
    rng = np.random.default_rng(3)
    r = Resident(rng, 336, True, True, True)
    nrm0, tan0, uv0 = r.nrm.copy(), r.tan.copy(), r.uv0.copy()
    pos = rng.uniform(-3, 3, (336, 3)).astype(np.float32)
    assert r.ingest(shim, pos)[0] == 0  # positions only
    assert same(r.pos, pos) and same(r.nrm, nrm0) and same(r.tan, tan0)
    assert same(r.verts, vu.interleave(pos, nrm0, uv0, tan0))
    tan = rng.normal(size=(336, 4)).astype(np.float32)
    assert r.ingest(shim, pos, None, tan)[0] == 0  # positions and tangents, no normals
    assert same(r.nrm, nrm0) and same(r.tan, tan) and same(r.verts, vu.interleave(pos, nrm0, uv0, tan))


# ---- rejection ----------------------------------------------------------------------------------------------------------------------------
def test_a_vertex_with_a_non_finite_component_keeps_all_its_resident_values(shim):
    rng = np.random.default_rng(5)
    nv = 336
    r = Resident(rng, nv, True, True, True)
    before = (r.pos.copy(), r.nrm.copy(), r.tan.copy(), r.verts.copy())
    pos = rng.uniform(-3, 3, (nv, 3)).astype(np.float32)
    nrm = rng.normal(size=(nv, 3)).astype(np.float32)
    tan = rng.normal(size=(nv, 4)).astype(np.float32)
    salt = {0: (pos, 0, np.nan), 63: (pos, 2, np.inf), 64: (nrm, 1, -np.inf), 255: (tan, 3, np.nan), 256: (tan, 0, np.inf), 335: (nrm, 2, np.nan),
            100: (pos, 1, -np.inf)}
    for v, (a, c, value) in salt.items():
        a[v, c] = value
    pos[200, 0] = np.float32(3.4e38)     # the largest magnitudes and a denormal are finite: written
    pos[201, 1] = np.float32(1e-45)
    n, rejected = r.ingest(shim, pos, nrm, tan)
    assert n == len(salt) and sorted(np.nonzero(rejected)[0]) == sorted(salt)
    keep = rejected
    for got, old, new in zip((r.pos, r.nrm, r.tan), before[:3], (pos, nrm, tan)):
        assert same(got[keep], old[keep]) and same(got[~keep], new[~keep])
    want = vu.interleave(pos, nrm, r.uv0, tan)
    assert same(r.verts[keep], before[3][keep]) and same(r.verts[~keep], want[~keep])
    assert np.isfinite(r.pos).all() and np.isfinite(r.nrm).all() and np.isfinite(r.tan).all()
    # a non-finite value in a stream the call does not supply cannot exist; one in a supplied stream rejects the vertex whatever the others hold
    r2 = Resident(rng, 4, True, False, False)
    p2 = np.ones((4, 3), np.float32)
    n2 = np.ones((4, 3), np.float32)
    n2[2, 0] = np.nan
    assert r2.ingest(shim, p2, n2)[0] == 1 and np.isfinite(r2.pos).all() and not same(r2.pos[2], p2[2])


# ---- the normal rebuild -------------------------------------------------------------------------------------------------------------------
def _rebuild(shim, pos, idx, resident):
    nv = len(pos)
    end, corners = vu.corner_table(idx, nv)
    nrm = np.ascontiguousarray(resident, np.float32).copy()
    verts = vu.interleave(pos, nrm)
    verts[:, 6:] = 7.0  # (uv0 and the tangent: must stay)
    idx = np.ascontiguousarray(idx, np.uint32)
    pos = np.ascontiguousarray(pos, np.float32)
    shim.dev_rebuild_normals(nv, fp(pos), idx.ctypes.data_as(P(U)), end.ctypes.data_as(P(U)), corners.ctypes.data_as(P(U)), fp(nrm), fp(verts))
    assert same(verts[:, 3:6], nrm) and same(verts[:, :3], pos) and (verts[:, 6:] == 7.0).all()
    return nrm


def _meshes():
    cp, _, _, ci = scenegen.grid(20, 15, (2.0, 1.5), axis="z")
    out = [("cloth wave %.1f" % ph, vu.cloth_wave(cp, ph)[0], ci) for ph in (0.0, 0.7, 2.1)]
    sp, sn, _, si = scenegen.uv_sphere(24, 12, 0.4)
    out.append(("ball", sp, si))
    out.append(("ball pulse", vu.ball_pulse(sp, sn, 0.4)[0], si))
    return out


def test_corner_table_lists_every_corner_once_in_ascending_order():
    _, _, _, idx = scenegen.uv_sphere(24, 12, 0.4)
    end, corners = vu.corner_table(idx, 325)
    assert end[-1] == idx.size and sorted(corners) == list(range(idx.size))
    start = np.concatenate([[0], end[:-1]])
    flat = idx.reshape(-1)
    for v in (0, 24, 25, 100, 324):
        run = corners[start[v]:end[v]]
        assert (flat[run] == v).all() and (np.diff(run.astype(np.int64)) > 0).all() and len(run) == (flat == v).sum()


def test_rebuilt_normals_match_the_float64_definition(shim):
    worst = 0.0
    for name, pos, idx in _meshes():
        resident = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (len(pos), 1))
        got = _rebuild(shim, pos, idx, resident)
        want, kept = vu.rebuilt_normals_f64(pos, idx, resident)
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        print("%-16s max |n - n64| = %.3g, vertices keeping their normal: %d" % (name, err, kept.sum()))
        assert err <= vu.NORMAL_BOUND, (name, err)
        assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() < 1e-6
        assert same(got[kept], resident[kept])
        if name == "ball":  # the sphere's own normals are radial: the rebuild finds them to mesh accuracy away from the seam and the poles
            radial = pos / np.linalg.norm(pos, axis=1, keepdims=True)
            assert np.abs(got - radial)[~kept].max() < 0.15
            # the last vertex of the north-pole row touches one zero-area triangle only.  (Its southern counterpart does not keep its normal:
            # sin(pi) is 1.2e-16 in floating point, that row's vertices differ, and its sliver has a direction both precisions agree on.)
            assert list(np.nonzero(kept)[0]) == [24]
    # the host-compiled function leaves the device's FMA contraction a factor of two inside the bound
    assert worst <= 1e-6, worst


def test_a_vertex_without_incident_area_keeps_its_resident_normal(shim):
    # vertices 0-2: a proper triangle; 3-5: a zero-area one (collinear); 6: no triangle at all; 7-9: two opposite triangles that cancel
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [9, 9, 9], [5, 0, 0], [6, 0, 0], [5, 1, 0]], np.float32)
    idx = np.array([[0, 1, 2], [3, 4, 5], [7, 8, 9], [7, 9, 8]], np.uint32)
    resident = np.tile(np.array([[0.6, 0.0, 0.8]], np.float32), (10, 1))
    got = _rebuild(shim, pos, idx, resident)
    assert same(got[:3], np.tile(np.array([[0, 0, 1]], np.float32), (3, 1)))
    assert same(got[3:], resident[3:])
    want, kept = vu.rebuilt_normals_f64(pos, idx, resident)
    assert list(np.nonzero(kept)[0]) == [3, 4, 5, 6, 7, 8, 9] and np.abs(got - want).max() == 0.0
    # an overflowing sum has no finite length: kept too
    big = np.array([[0, 0, 0], [3e19, 0, 0], [0, 3e19, 0]], np.float32)
    assert same(_rebuild(shim, big, idx[:1], resident[:3]), resident[:3])


# ---- public surface -----------------------------------------------------------------------------------------------------------------------
def test_vertex_update_entry_points_are_declared_bound_and_exported(built):
    from vk_gltf_renderer_amd import _capi as capi
    header = open(os.path.join(ROOT, "include", "mi_pt.h")).read()
    assert re.search(r"#define MI_PT_ABI_VERSION 9\b", header)
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vk_gltf_renderer_amd", "lib", "libmi_pt.so")], check=True,
                              capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(r"MI_PT_API\s+\w+\s+%s\(" % name, header), name
        assert name in capi.PT_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
    assert re.search(r"MI_PT_VERTICES_RECOMPUTE_NORMALS\s*=\s*1\b", header) and capi.MI_PT_VERTICES_RECOMPUTE_NORMALS == 1
    assert C.sizeof(capi.MiPtVertexUpdate) == 40 and C.sizeof(capi.MiPtVertexUpdateInfo) == 32
    assert capi.MI_PT_ABI_VERSION == 9 and capi.pt_lib().mi_pt_abi_version() == 9
    from vk_gltf_renderer_amd import pathtracer as ptmod
    for name in ("set_vertex_updates", "update_vertices", "vertex_update_info"):
        assert callable(getattr(ptmod.PathTracer, name))
    assert callable(scenegen.scene_dynamic)
