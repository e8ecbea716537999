"""The per-ray work of the _ex ray queries (csrc/device/pt_query.h, second half) compiled for the host through tests/host_shim -- no GPU needed:
the layout of MiPtQueryOptions (32 bytes; ABI still 9) and the new enum values, the three new entry points in the header, in the library and in
the Python binding, the cull rule, the alpha decision, the exact STOCHASTIC draw, and the brute force over hand-made and generated triangle
sets: the same records whatever the order the triangles are met in, slots listed twice (pre-split references) appearing once in a K-list,
default rules returning what the plain per-ray code returns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import query_ex_util as qx
import query_util as qu
from test_query_on_host import HITREC, make_ray, make_tris

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HIT, FRONT, INVALID = 1, 2, 4


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return qx.Shim(tmp_path_factory.mktemp("host_shim_query_ex"))


@pytest.fixture(scope="module")
def plain_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_shim_query_plain") / "libquery_on_host.so")
    d = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + d, "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"),
                    "-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(d, "query_on_host.cpp")], check=True)
    L = C.CDLL(out)
    L.query_brute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return L


def no_alpha(n):
    """Alpha records of n triangles of OPAQUE materials, and an empty texel pool."""
    rec = np.zeros(n, qx.ALPHA_DTYPE)
    rec["factor"], rec["cutoff"] = 1.0, 0.5
    return rec, np.zeros((1, 4), np.uint8)


def test_layout_enums_abi_and_symbols(shim):
    out = np.zeros(18, np.int32)
    shim.lib.query_ex_layout(out.ctypes.data)
    assert out[0] == 32 and list(out[1:8]) == [0, 4, 8, 12, 16, 20, 24]
    assert out[8] == 9
    assert list(out[9:18]) == [0, 1, 2, 0, 1, 2, 0, 1, 8]
    header = open(os.path.join(ROOT, "include", "mi_pt.h")).read()
    assert re.search(r"#define MI_PT_ABI_VERSION 9\b", header)
    from vk_gltf_renderer_amd import _capi as capi
    assert capi.MI_PT_ABI_VERSION == 9
    assert C.sizeof(capi.MiPtQueryOptions) == 32
    assert [getattr(capi.MiPtQueryOptions, n).offset for n, _ in capi.MiPtQueryOptions._fields_] == list(out[1:8])
    assert (capi.MI_PT_QUERY_NEAREST_K, capi.MI_PT_QUERY_ALPHA_CUTOFF, capi.MI_PT_QUERY_ALPHA_STOCHASTIC, capi.MI_PT_QUERY_CULL_MATERIAL,
            capi.MI_PT_QUERY_MAX_HITS) == (2, 1, 2, 1, 8)
    lib = capi.pt_lib()
    assert lib.mi_pt_abi_version() == 9
    for name in ("mi_pt_query_rays_ex", "mi_pt_query_rays_device_ex", "mi_pt_pick_ex"):
        assert re.search(r"MI_PT_API int %s\(" % name, header), name
        assert name in capi.PT_SYMBOLS and getattr(lib, name) is not None, name
    assert "mi_pt_default_query_options" in capi.PT_SYMBOLS
    o = capi.MiPtQueryOptions()
    C.memset(C.byref(o), 0xAB, 32)
    lib.mi_pt_default_query_options(C.byref(o))
    assert (o.mode, o.alpha, o.cull, o.maxHits, o.blendThreshold, o.seed, o.reserved[0], o.reserved[1]) == (0, 0, 0, 1, 0.5, 0, 0, 0)
    assert qx.RULES_DTYPE.itemsize == 20


def test_cull_rule_alpha_decision_and_draw(shim):
    L = shim.lib
    for flags in range(32):
        for front in (0, 1):
            assert L.query_ex_cull_passes(flags, front, qx.CULL_NONE) == 1
            object_front = bool(front) != bool(flags & qx.INST_FLIP_FACING)
            assert L.query_ex_cull_passes(flags, front, qx.CULL_MATERIAL) == int(object_front or bool(flags & qx.INST_CULL_DISABLE)), (flags, front)
    # CUTOFF: opacity >= threshold; STOCHASTIC: draw <= opacity
    assert L.query_ex_alpha_decision(qx.CUTOFF, 0.5, 0.5, 0.99) == 1 and L.query_ex_alpha_decision(qx.CUTOFF, np.nextafter(F32(0.5), F32(0)), 0.5, 0.0) == 0
    assert L.query_ex_alpha_decision(qx.CUTOFF, 1.0, 1.0, 0.0) == 1 and L.query_ex_alpha_decision(qx.CUTOFF, 0.0, 1e-6, 0.0) == 0
    assert L.query_ex_alpha_decision(qx.STOCHASTIC, 0.25, 0.9, 0.25) == 1 and L.query_ex_alpha_decision(qx.STOCHASTIC, 0.25, 0.1, np.nextafter(F32(0.25), F32(1))) == 0
    assert L.query_ex_alpha_decision(qx.STOCHASTIC, 0.0, 0.5, 0.0) == 1 and L.query_ex_alpha_decision(qx.STOCHASTIC, 1.0, 0.5, np.nextafter(F32(1), F32(0))) == 1
    # the draw: query_ex_util.draw is the device's, exactly
    rng = np.random.default_rng(5)
    seed, ray, node, prim = (rng.integers(0, 2 ** 32, 500, dtype=np.uint64) for _ in range(4))
    ray[:50], node[:50], prim[:50] = np.arange(50), 3, np.arange(50)
    want = qx.draw(seed, ray, node, prim)
    got = np.array([L.query_ex_draw(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(seed, ray, node, prim)])
    assert (got == want).all() and (0 <= got).all() and (got < 1).all()
    assert len(np.unique(got)) > 490  # (and it depends on every argument)
    assert L.query_ex_draw(1, 2, 3, 4) != L.query_ex_draw(2, 2, 3, 4) != L.query_ex_draw(2, 3, 3, 4) != L.query_ex_draw(2, 3, 4, 4) != L.query_ex_draw(2, 3, 4, 5)


def _stack():
    """Five triangles over the unit square corner at z = 0, -1, ..., -4: render node 1 + i, triangle 10 + i; every second one wound clockwise seen
    from +z.  Slot 5 repeats slot 1, slot 6 repeats slot 3 (pre-split references of one triangle)."""
    rows = []
    for i in range(5):
        a, b, c = (0, 0, -i), (1, 0, -i), (0, 1, -i)
        rows.append((a, b, c, 1 + i, 10 + i, 0) if i % 2 == 0 else (a, c, b, 1 + i, 10 + i, 0))
    tris, shade = make_tris(rows)
    tris, shade = np.concatenate([tris, tris[[1, 3]]]), np.concatenate([shade, shade[[1, 3]]])
    return tris, shade


def test_k_lists_are_sorted_distinct_and_independent_of_the_order(shim):
    tris, shade = _stack()
    alpha, texels = no_alpha(len(tris))
    ray = make_ray((0.25, 0.25, 2), (0, 0, -1))
    rng = np.random.default_rng(2)
    orders = [np.arange(7), np.arange(7)[::-1], np.array([5, 1, 6, 3, 0, 2, 4])] + [rng.permutation(7) for _ in range(20)]
    for k in range(1, 9):
        first = shim.brute(tris, shade, alpha, texels, ray, qx.rules(max_hits=k), order=orders[0])
        want = min(k, 5)
        assert first.shape == (1, k) and list(first["renderNode"][0, :want]) == [1, 2, 3, 4, 5][:want] and list(first["t"][0, :want]) == [2, 3, 4, 5, 6][:want]
        assert (first["renderNode"][0, want:] == -1).all() and (first["flags"][0, want:] == 0).all() and not first["t"][0, want:].any()
        for order in orders[1:]:
            got = shim.brute(tris, shade, alpha, texels, ray, qx.rules(max_hits=k), order=order)
            assert got.tobytes() == first.tobytes(), (k, order)
    # culling: the clockwise triangles show this ray their back
    culled = shim.brute(tris, shade, alpha, texels, ray, qx.rules(max_hits=8, cull=qx.CULL_MATERIAL), order=orders[2])
    assert list(culled["renderNode"][0, :4]) == [1, 3, 5, -1] and ((culled["flags"][0, :3] & FRONT) != 0).all()
    up = make_ray((0.25, 0.25, -9), (0, 0, 1))
    assert list(shim.brute(tris, shade, alpha, texels, up, qx.rules(max_hits=4, cull=qx.CULL_MATERIAL))["renderNode"][0]) == [4, 2, -1, -1]
    for flag, want in ((qx.INST_CULL_DISABLE, [1, 2, 3, 4, 5]), (qx.INST_FLIP_FACING, [2, 4, -1, -1, -1])):
        t2 = tris.copy()
        t2["flags"] = flag
        assert list(shim.brute(t2, shade, alpha, texels, ray, qx.rules(max_hits=5, cull=qx.CULL_MATERIAL))["renderNode"][0]) == want, flag
    # exact ties go by (renderNode, triangle), and tMin = the last t skips the whole tie group
    flat, fshade = make_tris([((0, 0, 0), (1, 0, 0), (0, 1, 0), n, p, 0) for n, p in ((3, 5), (3, 2), (1, 9), (2, 0))])
    fa, ft = no_alpha(4)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2]):
        got = shim.brute(flat, fshade, fa, ft, ray, qx.rules(max_hits=3), order=order)
        assert list(zip(got["renderNode"][0], got["triangle"][0])) == [(1, 9), (2, 0), (3, 2)] and (got["t"][0] == 2.0).all()
    assert shim.brute(flat, fshade, fa, ft, make_ray((0.25, 0.25, 2), (0, 0, -1), tmin=2.0), qx.rules(max_hits=3))["renderNode"][0, 0] == -1
    # an invalid ray: its first record says so, the others are plain misses
    bad = shim.brute(tris, shade, alpha, texels, make_ray((np.nan, 0, 2), (0, 0, -1)), qx.rules(max_hits=4))
    assert list(bad["flags"][0]) == [INVALID, 0, 0, 0] and (bad["renderNode"][0] == -1).all()
    z = bad.copy()
    z["flags"], z["renderNode"] = 0, 0
    assert not z.view(np.uint8).any()


def test_alpha_modes_on_hand_made_records(shim):
    """Four stacked triangles: OPAQUE material, BLEND with factor 0.6, MASK with vertex alphas 255 / 0 / 0 against cutoff 0.5, BLEND behind
    a nearest-filtered 2 x 1 texture with alphas 0 and 255."""
    rows = [((0, 0, -i), (1, 0, -i), (0, 1, -i), i, 0, f) for i, f in enumerate((qx.INST_FORCE_OPAQUE, 0, 0, 0))]
    tris, shade = make_tris(rows)
    alpha, _ = no_alpha(4)
    alpha["flags"][1], alpha["factor"][1] = qx.ALPHA_BLEND, 0.6
    alpha["flags"][2], alpha["colors"][2] = qx.ALPHA_MASK | qx.AT_HAS_COLORS, 255
    alpha["flags"][3] = qx.ALPHA_BLEND | qx.AT_HAS_TEXTURE
    alpha["uv0"][3], alpha["uv1"][3], alpha["uv2"][3], alpha["size"][3] = (0, 0), (1, 0), (0, 1), 2 | (1 << 16)
    texels = np.array([[9, 9, 9, 0], [9, 9, 9, 255]], np.uint8)
    L = shim.lib
    assert L.query_ex_opacity(alpha.ctypes.data, texels.ctypes.data, 0, 0.2, 0.2) == 1.0
    assert L.query_ex_opacity(alpha.ctypes.data, texels.ctypes.data, 1, 0.2, 0.2) == F32(0.6)
    assert L.query_ex_opacity(alpha.ctypes.data, texels.ctypes.data, 2, 0.2, 0.2) == 1.0 and L.query_ex_opacity(alpha.ctypes.data, texels.ctypes.data, 2, 0.3, 0.3) == 0.0
    assert L.query_ex_opacity(alpha.ctypes.data, texels.ctypes.data, 3, 0.2, 0.2) == 0.0 and L.query_ex_opacity(alpha.ctypes.data, texels.ctypes.data, 3, 0.7, 0.2) == 1.0
    near, far = make_ray((0.2, 0.2, 2), (0, 0, -1), tmin=2.5), make_ray((0.3, 0.3, 2), (0, 0, -1), tmin=2.5)  # (tMin: behind the opaque triangle)
    right = make_ray((0.7, 0.2, 2), (0, 0, -1), tmin=2.5)
    nodes = lambda ray, **kw: list(shim.brute(tris, shade, alpha, texels, ray, qx.rules(max_hits=4, **kw))["renderNode"][0])
    assert nodes(near) == [1, 2, 3, -1]  # OPAQUE: every triangle counts
    assert nodes(near, alpha=qx.CUTOFF, blend_threshold=0.5) == [1, 2, -1, -1]   # 0.6 >= 0.5; vertex alpha 0.6 >= cutoff; texel 0
    assert nodes(near, alpha=qx.CUTOFF, blend_threshold=0.7) == [2, -1, -1, -1]  # the MASK triangle follows its own cutoff
    assert nodes(far, alpha=qx.CUTOFF, blend_threshold=0.5) == [1, -1, -1, -1]   # vertex alpha 0.4 < cutoff
    assert nodes(right, alpha=qx.CUTOFF, blend_threshold=1.0) == [3, -1, -1, -1]  # texel 255: opacity 1 >= 1
    assert shim.brute(tris, shade, alpha, texels, make_ray((0.2, 0.2, 2), (0, 0, -1)), qx.rules(alpha=qx.CUTOFF, blend_threshold=0.99))["renderNode"][0, 0] == 0
    # STOCHASTIC: the BLEND triangle is accepted iff the exact draw of (seed, ray index, node 1, triangle 0) is <= 0.6; about 60 % of the rays
    rays = np.repeat(near, 400)
    got = shim.brute(tris, shade, alpha, texels, rays, qx.rules(alpha=qx.STOCHASTIC, seed=77))[:, 0]
    want = qx.draw(77, np.arange(400), 1, 0) <= float(F32(0.6))
    assert ((got["renderNode"] == 1) == want).all() and (got["renderNode"][~want] == 2).all()
    assert 0.5 < want.mean() < 0.7
    again = shim.brute(tris, shade, alpha, texels, rays, qx.rules(alpha=qx.STOCHASTIC, seed=77))[:, 0]
    other = shim.brute(tris, shade, alpha, texels, rays, qx.rules(alpha=qx.STOCHASTIC, seed=78))[:, 0]
    assert again.tobytes() == got.tobytes() and other.tobytes() != got.tobytes()
    shifted = shim.brute(tris, shade, alpha, texels, rays[:100], qx.rules(alpha=qx.STOCHASTIC, seed=77), first=300)[:, 0]
    assert shifted.tobytes() == got[300:].tobytes()  # keyed on the ray's index in the call
    # ANY under an alpha mode: a hit iff CLOSEST has one
    assert shim.brute(tris, shade, alpha, texels, far, qx.rules(alpha=qx.CUTOFF), any_hit=True, order=[3, 2, 1, 0])["renderNode"][0, 0] == 1


def test_generated_scene_shuffled_orders_duplicates_and_default_rules(shim, plain_lib, tmp_path):
    from vk_gltf_renderer_amd import pathtracer as ptmod
    scene = ptmod.Scene(qx.make_scene("mixed_alpha_glass", tmp_path))
    st = qu.SceneTris(scene)
    sa = qx.SceneAlpha(scene, st)
    rays = qx.make_rays_ex(st, sa, n=128)
    tris, shade, alpha, texels = qx.shim_records(st, sa)
    n = len(tris)
    rng = np.random.default_rng(9)
    # default rules: the plain per-ray code's records, bit for bit
    plain = np.zeros(len(rays), HITREC)
    order = np.arange(n, dtype=np.int32)
    for i in range(len(rays)):
        plain_lib.query_brute(tris.ctypes.data, shade.ctypes.data, order.ctypes.data, n, rays[i:i + 1].ctypes.data, 0, plain[i:i + 1].ctypes.data)
    assert shim.brute(tris, shade, alpha, texels, rays, qx.rules()).tobytes() == plain.tobytes()
    assert shim.brute(tris, shade, alpha, texels, rays, qx.rules(max_hits=1)).tobytes() == plain.tobytes()
    # every tenth slot listed twice more, at the end and in the middle of a shuffled order
    dup = np.arange(0, n, 10)
    for kw in (dict(), dict(alpha=qx.CUTOFF, cull=qx.CULL_MATERIAL), dict(alpha=qx.STOCHASTIC, seed=4), dict(alpha=qx.CUTOFF, blend_threshold=0.9, max_hits=3),
               dict(alpha=qx.STOCHASTIC, seed=4, cull=qx.CULL_MATERIAL, max_hits=8)):
        base = shim.brute(tris, shade, alpha, texels, rays, qx.rules(**kw))
        for _ in range(3):
            order = rng.permutation(np.concatenate([np.arange(n), dup, dup]))
            got = shim.brute(tris, shade, alpha, texels, rays, qx.rules(**kw), order=order)
            assert got.tobytes() == base.tobytes(), kw
        k = kw.get("max_hits", 1)
        if k > 1:
            hit = base["renderNode"] >= 0
            assert hit[:, 1].any()
            for i in range(len(rays)):
                ids = list(zip(base["renderNode"][i][hit[i]], base["triangle"][i][hit[i]]))
                assert len(set(ids)) == len(ids)
    # the opacity the device computes against float64, on the tested triangles
    k = rng.permutation(np.nonzero(sa.tested)[0])[:300]
    u, v = rng.uniform(0, 0.5, len(k)), rng.uniform(0, 0.5, len(k))
    got = np.array([shim.lib.query_ex_opacity(alpha.ctypes.data, texels.ctypes.data, int(a), F32(b), F32(c)) for a, b, c in zip(k, u, v)])
    raw = sa.alpha(k, u.astype(F32).astype(np.float64), v.astype(F32).astype(np.float64))
    blend = sa.mode[k] == qx.ALPHA_BLEND
    assert blend.any() and (~blend).any()
    assert np.abs(got[blend] - raw[blend]).max() < 1e-6
    sure = ~blend & (np.abs(raw - sa.cutoff[k]) > qx.ALPHA_BAND)
    assert (got[sure] == (raw[sure] >= sa.cutoff[k][sure])).all()
    scene.close()
