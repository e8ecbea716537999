"""The per-ray work of the ray queries (csrc/device/pt_query.h) compiled for the host through tests/host_shim -- no GPU needed: the layout of
MiPtRay / MiPtRayHit (include/mi_pt.h, ABI still 9), ray validation, the acceptance interval, the closest-hit rule with its tie-break, and
fillHit on hand-made triangle and shade records (position = fma(t, direction, origin), a unit normal that faces the ray for both windings, the
front-face bit under INST_FLIP_FACING, ids copied from the shade record, the miss record)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HIT, FRONT, INVALID = 1, 2, 4
FLIP_FACING = 4  # pt_scene.h: INST_FLIP_FACING

RAY = np.dtype([("origin", "<f4", (3,)), ("tMin", "<f4"), ("direction", "<f4", (3,)), ("tMax", "<f4")])
HITREC = np.dtype([("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("flags", "<u4"), ("renderNode", "<i4"), ("renderPrimID", "<i4"), ("triangle", "<u4"),
                   ("materialID", "<i4"), ("position", "<f4", (3,)), ("reserved0", "<f4"), ("normal", "<f4", (3,)), ("reserved1", "<f4")])
# DevTri {v0, rnode} {e1, prim} {e2, instFlags}; DevShadeTri (pt_scene.h)
TRI = np.dtype([("v0", "<f4", (3,)), ("rnode", "<u4"), ("e1", "<f4", (3,)), ("prim", "<u4"), ("e2", "<f4", (3,)), ("flags", "<u4")])
SHADE = np.dtype([("v0", "<u4"), ("v1", "<u4"), ("v2", "<u4"), ("rnode", "<u4"), ("renderPrimID", "<i4"), ("materialID", "<i4"), ("prim", "<u4"),
                  ("attrs", "<u4")])


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_shim_query") / "libquery_on_host.so")
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + shim, "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"),
                    "-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(shim, "query_on_host.cpp")], check=True)
    L = C.CDLL(out)
    VP, I, F = C.c_void_p, C.c_int, C.c_float
    L.query_layout.argtypes = [VP]
    L.query_ray_valid.argtypes = [VP]
    L.query_ray_valid.restype = I
    L.query_accept.argtypes = [F, F, F]
    L.query_accept.restype = I
    L.query_tmin.argtypes = [F]
    L.query_tmin.restype = F
    L.query_ray_setup.argtypes = [VP, VP]
    L.query_miss.argtypes = [C.c_uint32, VP]
    L.query_fill_hit.argtypes = [VP, VP, I, F, F, F, I, VP, VP]
    L.query_brute.argtypes = [VP, VP, VP, I, VP, I, VP]
    return L


def make_ray(o, d, tmin=0.0, tmax=np.inf):
    r = np.zeros(1, RAY)
    r["origin"], r["direction"], r["tMin"], r["tMax"] = o, d, tmin, tmax
    return r


def make_tris(rows):
    """rows: (v0, v1, v2, rnode, prim, flags) -> (DevTri array, DevShadeTri array with ids that differ from the triangle record's on purpose)."""
    t, s = np.zeros(len(rows), TRI), np.zeros(len(rows), SHADE)
    for i, (v0, v1, v2, rnode, prim, flags) in enumerate(rows):
        v0, v1, v2 = (np.asarray(x, F32) for x in (v0, v1, v2))
        t[i] = (v0, rnode, v1 - v0, prim, v2 - v0, flags)
        s[i] = (100 + i, 200 + i, 300 + i, rnode, 40 + i, 7 + i, prim, 0)
    return t, s


def fill(lib, tris, shade, i, t, u, v, front, ray):
    out = np.zeros(1, HITREC)
    lib.query_fill_hit(tris.ctypes.data, shade.ctypes.data, i, t, u, v, int(front), ray.ctypes.data, out.ctypes.data)
    return out[0]


def brute(lib, tris, shade, ray, any_hit=False, order=None):
    order = np.arange(len(tris), dtype=np.int32) if order is None else np.asarray(order, np.int32)
    out = np.zeros(1, HITREC)
    lib.query_brute(tris.ctypes.data, shade.ctypes.data, order.ctypes.data, len(order), ray.ctypes.data, int(any_hit), out.ctypes.data)
    return out[0]


def test_layout_is_the_headers_and_the_abi_version_stays_9(lib):
    out = np.zeros(24, np.int32)
    lib.query_layout(out.ctypes.data)
    assert out[0] == 32 and list(out[1:5]) == [0, 12, 16, 28]
    assert out[5] == 64 and list(out[6:18]) == [0, 4, 8, 12, 16, 20, 24, 28, 32, 44, 48, 60]
    assert out[18] == 9
    assert list(out[19:24]) == [1, 2, 4, 0, 1]
    assert RAY.itemsize == 32 and HITREC.itemsize == 64
    assert [HITREC.fields[n][1] for n in HITREC.names] == list(out[6:18])
    header = open(os.path.join(ROOT, "include", "mi_pt.h")).read()
    assert re.search(r"#define MI_PT_ABI_VERSION 9\b", header)
    for name in ("mi_pt_query_rays", "mi_pt_query_rays_device", "mi_pt_pick"):
        assert re.search(r"MI_PT_API int %s\(" % name, header), name
    # the Python mirror of the records
    from vk_gltf_renderer_amd import _capi as capi
    from vk_gltf_renderer_amd import pathtracer as ptmod
    assert C.sizeof(capi.MiPtRay) == 32 and C.sizeof(capi.MiPtRayHit) == 64
    assert [getattr(capi.MiPtRayHit, n).offset for n in HITREC.names] == list(out[6:18])
    assert ptmod.HIT_DTYPE == HITREC


def test_ray_validation(lib):
    ok = make_ray((1, 2, 3), (0, 0, 1))
    assert lib.query_ray_valid(ok.ctypes.data) == 1
    assert lib.query_ray_valid(make_ray((1, 2, 3), (0, 0, 1), tmin=-np.inf, tmax=np.inf).ctypes.data) == 1  # infinite bounds are bounds
    for bad in (np.nan, np.inf, -np.inf):
        for field in ("origin", "direction"):
            for axis in range(3):
                r = make_ray((1, 2, 3), (0.5, 0.5, 1))
                r[field][0, axis] = bad
                assert lib.query_ray_valid(r.ctypes.data) == 0, (bad, field, axis)
    assert lib.query_ray_valid(make_ray((0, 0, 0), (0, 0, 0)).ctypes.data) == 0
    assert lib.query_ray_valid(make_ray((0, 0, 0), (0.0, -0.0, 0.0)).ctypes.data) == 0
    assert lib.query_ray_valid(make_ray((0, 0, 0), (0, 0, 1), tmin=np.nan).ctypes.data) == 0
    assert lib.query_ray_valid(make_ray((0, 0, 0), (0, 0, 1), tmax=np.nan).ctypes.data) == 0
    # denormal direction components: accepted, and makeRaySetup turns them into finite reciprocals
    with np.errstate(under="ignore"):
        den = F32(1e-41)
    for d in ((den, 0, 0), (den, -den, den), (0, 1, den)):
        r = make_ray((1, 2, 3), d)
        assert lib.query_ray_valid(r.ctypes.data) == 1, d
        out = np.zeros(6, F32)
        lib.query_ray_setup(r.ctypes.data, out.ctypes.data)
        assert np.isfinite(out).all(), (d, out)
        assert (np.abs(out[:3]) <= 1e30 * 1.0001).all()


def test_acceptance_is_the_open_interval(lib):
    tmin, tmax = F32(0.25), F32(4.0)
    assert lib.query_accept(tmin, tmin, tmax) == 0
    assert lib.query_accept(tmax, tmin, tmax) == 0
    assert lib.query_accept(np.nextafter(tmin, F32(1)), tmin, tmax) == 1
    assert lib.query_accept(np.nextafter(tmax, F32(0)), tmin, tmax) == 1
    assert lib.query_accept(np.nextafter(tmin, F32(0)), tmin, tmax) == 0
    assert lib.query_accept(np.nextafter(tmax, F32(8)), tmin, tmax) == 0
    assert lib.query_accept(F32(1e30), F32(0), F32(np.inf)) == 1
    assert lib.query_accept(F32(np.nan), tmin, tmax) == 0
    # nothing behind the origin: a negative tMin acts as 0
    assert lib.query_tmin(F32(-3.0)) == 0.0 and lib.query_tmin(F32(0.5)) == 0.5 and lib.query_tmin(F32(-np.inf)) == 0.0


def test_miss_record_is_zero_but_for_the_node(lib):
    for flags in (0, INVALID):
        out = np.zeros(1, HITREC)
        out.view(np.uint8)[:] = 0xAB
        lib.query_miss(flags, out.ctypes.data)
        words = out.view(np.uint32).copy()
        assert out["renderNode"][0] == -1 and out["flags"][0] == flags
        words[3] = 0
        words[4] = 0
        assert not words.any()


def test_fill_hit_position_normal_ids_and_front_face(lib):
    rng = np.random.default_rng(3)
    for case in range(200):
        v = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 3)
        flags = int(rng.integers(0, 32))
        tris, shade = make_tris([(v[0], v[1], v[2], 5, 9, flags)])
        o = rng.normal(size=3).astype(F32) * 5
        d = (rng.normal(size=3) * 10.0 ** rng.uniform(-2, 2)).astype(F32)
        ray = make_ray(o, d)
        t, b1, b2 = F32(rng.uniform(0.01, 50)), F32(0.25), F32(0.5)
        n64 = np.cross(tris["e1"][0].astype(np.float64), tris["e2"][0].astype(np.float64))
        n64 /= np.linalg.norm(n64)
        for front in (False, True):
            h = fill(lib, tris, shade, 0, t, b1, b2, front, ray)
            assert h["t"] == t and h["b1"] == b1 and h["b2"] == b2
            # position: ONE rounding per component (the float64 product of two floats is exact, so float64 then float32 is the fma but for double rounding)
            want = (np.float64(t) * d.astype(np.float64) + o.astype(np.float64))
            assert np.abs(h["position"].astype(np.float64) - want).max() <= np.abs(want).max() * 2.0 ** -23
            exact = np.array([np.float32(np.float64(t) * np.float64(d[k]) + np.float64(o[k])) for k in range(3)])
            assert (np.abs(h["position"] - exact) <= np.spacing(np.abs(exact))).all()
            # unit geometric normal, turned against the ray whatever the winding says
            n = h["normal"].astype(np.float64)
            assert abs(np.linalg.norm(n) - 1.0) < 4e-7
            assert np.dot(h["normal"], d) <= 0.0
            assert abs(abs(np.dot(n, n64)) - 1.0) < 1e-5
            # the front-face bit: the world-space winding bit, inverted by INST_FLIP_FACING and by nothing else
            assert bool(h["flags"] & HIT) and not (h["flags"] & INVALID)
            assert bool(h["flags"] & FRONT) == (front != bool(flags & FLIP_FACING)), (front, flags)
            # ids come from the SHADE record
            assert (h["renderNode"], h["renderPrimID"], h["triangle"], h["materialID"]) == (5, 40, 9, 7)
            assert h["reserved0"] == 0 and h["reserved1"] == 0
    # fma, not multiply-then-add: a product whose low bits the sum keeps
    t, dx, ox = F32(1.0 + 2.0 ** -12), F32(1.0 + 2.0 ** -12), F32(-1.0)
    tris, shade = make_tris([((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, 0, 0)])
    h = fill(lib, tris, shade, 0, t, 0.1, 0.1, True, make_ray((ox, 0, 0), (dx, 0, -1)))
    assert h["position"][0] == F32(2.0 ** -11 + 2.0 ** -24)
    assert F32(t * dx) + ox != h["position"][0]


def test_both_windings_face_the_ray_and_differ_in_the_front_bit(lib):
    a, b, c = (0, 0, 0), (1, 0, 0), (0, 1, 0)  # counter-clockwise seen from +z: normal +z
    for flags in (0, FLIP_FACING):
        tris, shade = make_tris([(a, b, c, 0, 0, flags), (a, c, b, 1, 0, flags)])
        down, up = make_ray((0.25, 0.25, 2), (0, 0, -1)), make_ray((0.25, 0.25, -2), (0, 0, 1))
        for ray, nz in ((down, 1.0), (up, -1.0)):
            for i in (0, 1):
                h = brute(lib, tris[i:i + 1], shade[i:i + 1], ray)
                assert h["flags"] & HIT and h["t"] == 2.0
                assert list(h["normal"]) == [0.0, 0.0, nz]
                world_front = (nz > 0) == (i == 0)  # the CCW triangle faces +z, its mirror -z
                assert bool(h["flags"] & FRONT) == (world_front != bool(flags)), (flags, nz, i)
                assert np.allclose(h["position"], (0.25, 0.25, 0.0))
                assert (h["b1"], h["b2"]) == ((0.25, 0.25))


def test_closest_rule_ties_bounds_and_any(lib):
    quad = lambda z, rnode, prim: ((0, 0, z), (1, 0, z), (0, 1, z), rnode, prim, 0)
    # two coincident triangles at z = 0 (a tie), one behind at z = -1
    tris, shade = make_tris([quad(0, 3, 5), quad(0, 3, 2), quad(0, 1, 9), quad(-1, 0, 0)])
    ray = make_ray((0.25, 0.25, 2), (0, 0, -1))
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2]):
        h = brute(lib, tris, shade, ray, order=order)
        assert (h["renderNode"], h["triangle"], h["t"]) == (1, 9, 2.0), order  # smallest (renderNode, triangle) among the tie
    # ... and within one render node the smaller triangle
    h = brute(lib, tris[:2], shade[:2], ray)
    assert (h["renderNode"], h["triangle"]) == (3, 2)
    # tMax at the hit distance: not accepted there, the walk finds nothing nearer; just beyond: accepted
    assert brute(lib, tris, shade, make_ray((0.25, 0.25, 2), (0, 0, -1), tmax=2.0))["renderNode"] == -1
    assert brute(lib, tris, shade, make_ray((0.25, 0.25, 2), (0, 0, -1), tmax=np.nextafter(F32(2), F32(3))))["renderNode"] == 1
    # tMin at the hit distance: the tie group is skipped, the triangle behind it is the closest
    h = brute(lib, tris, shade, make_ray((0.25, 0.25, 2), (0, 0, -1), tmin=2.0))
    assert (h["renderNode"], h["t"]) == (0, 3.0)
    assert brute(lib, tris, shade, make_ray((0.25, 0.25, 2), (0, 0, -1), tmin=np.nextafter(F32(2), F32(0))))["renderNode"] == 1
    # t is in units of |direction|
    h = brute(lib, tris, shade, make_ray((0.25, 0.25, 2), (0, 0, -4)))
    assert h["t"] == 0.5 and np.allclose(h["position"], (0.25, 0.25, 0))
    # ANY: the first accepted triangle in walk order, and a hit iff CLOSEST has one
    assert brute(lib, tris, shade, ray, any_hit=True, order=[3, 0, 1, 2])["renderNode"] == 0
    assert brute(lib, tris, shade, make_ray((5, 5, 2), (0, 0, -1)), any_hit=True)["flags"] == 0
    # a miss, an invalid ray, and a ray that starts beyond everything
    m = brute(lib, tris, shade, make_ray((5, 5, 2), (0, 0, -1)))
    assert m["renderNode"] == -1 and m["flags"] == 0 and not m["position"].any() and m["t"] == 0
    bad = brute(lib, tris, shade, make_ray((np.nan, 0, 2), (0, 0, -1)))
    assert bad["renderNode"] == -1 and bad["flags"] == INVALID
    assert brute(lib, tris, shade, make_ray((0.25, 0.25, -3), (0, 0, -1)))["renderNode"] == -1
    # a degenerate slot (a hidden node's in resident mode) is never hit
    tris, shade = make_tris([((0, 0, 0), (0, 0, 0), (0, 0, 0), 0, 0, 0)])
    assert brute(lib, tris, shade, make_ray((0, 0, 2), (0, 0, -1)))["renderNode"] == -1
