"""CPU tier: the debug views of MiSceneFrameInfo.visualization (csrc/device/pt_visualize.h: applyVisualization, hashToColor)
compiled for the host through tests/host_shim and diffed against a numpy restatement of the reference's definitions
(shaders/common.h.slang:32-164) on seeded random materials: every mode, the values outside the enum, clay's in-place material.
hashToColor must agree bit for bit, the rest within a few ulp (g++ -ffp-contract=off, libm pow)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vk_gltf_renderer_amd._capi import MI_VIZ_COUNT, Visualization as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, P = C.c_float, C.POINTER
FIELDS = ("baseColor", 3), ("opacity", 1), ("roughness", 2), ("metallic", 1), ("emissive", 3), ("occlusion", 1), ("N", 3), ("T", 3), ("B", 3), \
    ("Ng", 3), ("specular", 1), ("specularColor", 3), ("transmission", 1), ("clearcoat", 1), ("clearcoatRoughness", 1), ("Nc", 3), ("iridescence", 1), \
    ("iridescenceThickness", 1), ("sheenColor", 3), ("sheenRoughness", 1), ("diffuseTransmissionFactor", 1), ("diffuseTransmissionColor", 3)
RENDERED, COLOR_OVERRIDE, MATERIAL_OVERRIDE = 0, 1, 2


@pytest.fixture(scope="module")
def viz(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("viz_shim") / "libvisualize_on_host.so")
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-I" + shim, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"), "-o", out, os.path.join(shim, "visualize_on_host.cpp")], check=True)
    L = C.CDLL(out)
    L.dev_viz_material_layout.argtypes, L.dev_viz_material_layout.restype = [P(C.c_int)], C.c_int
    L.dev_apply_visualization.argtypes = [P(F), P(F), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(F)]
    L.dev_apply_visualization.restype = C.c_int
    L.dev_hash_to_color.argtypes = [C.c_uint32, P(F)]
    offs = (C.c_int * len(FIELDS))()
    L.n_floats = L.dev_viz_material_layout(offs)
    L.offsets = {name: (int(o), n) for (name, n), o in zip(FIELDS, offs)}
    return L


def _unit(rng):
    v = rng.normal(size=3)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _material(L, rng):
    m = {name: rng.uniform(0.0, 1.0, n).astype(np.float32) for name, n in FIELDS}
    for k in ("N", "T", "B", "Ng", "Nc"):
        m[k] = _unit(rng)
    m["iridescenceThickness"] = rng.uniform(50.0, 1200.0, 1).astype(np.float32)
    if rng.uniform() < 0.5:  # anisotropic: roughness.x inflated above roughness.y
        m["roughness"] = np.sort(m["roughness"])[::-1].copy()
    if rng.uniform() < 0.2:  # tiny values: the linear branch of the sRGB curve
        m["baseColor"] = rng.uniform(0.0, 0.004, 3).astype(np.float32)
    arr = np.zeros(L.n_floats, np.float32)
    for name, (o, n) in L.offsets.items():
        arr[o:o + n] = m[name]
    return m, arr


def _srgb(c):
    c = np.asarray(c, np.float32)
    p = np.power(c, np.float32(1.0 / 2.4))
    hi = (p.astype(np.float64) * np.float64(np.float32(1.055)) + np.float64(np.float32(-0.055))).astype(np.float32)  # one rounding, as fmaf
    return np.where(c > np.float32(0.0031308), hi, c * np.float32(12.92)).astype(np.float32)


def _hash_to_color(i):
    h = np.uint32(i)
    with np.errstate(over="ignore"):
        h = np.uint32(h * np.uint32(747796405) + np.uint32(2891336453))
        h = np.uint32((np.uint32(h >> np.uint32((h >> np.uint32(28)) + np.uint32(4))) ^ h) * np.uint32(277803737))
        h = np.uint32((h >> np.uint32(22)) ^ h)
    return np.array([(h >> s) & 0xFF for s in (0, 8, 16)], np.float32) / np.float32(255.0)


def expected(mode, m, uv, front, rprim, prim, omm):
    """numpy restatement of applyVisualization: (result, colour or None)."""
    half = np.float32(0.5)
    s3 = lambda x: np.full(3, np.float32(x[0] if np.ndim(x) else x), np.float32)  # noqa: E731
    r = m["roughness"]
    fract = lambda x: (x - np.floor(x)).astype(np.float32)  # noqa: E731
    table = {
        V.BASE_COLOR: lambda: _srgb(m["baseColor"]),
        V.METALLIC: lambda: _srgb(s3(m["metallic"])),
        V.ROUGHNESS: lambda: _srgb(np.array([r[0], r[1], r[0]], np.float32)),
        V.NORMAL_SHADING: lambda: _srgb(m["N"] * half + half),
        V.NORMAL_GEOMETRIC: lambda: m["Ng"] * half + half,
        V.TANGENT: lambda: m["T"] * half + half,
        V.BITANGENT: lambda: m["B"] * half + half,
        V.EMISSIVE: lambda: m["emissive"],
        V.OPACITY: lambda: s3(m["opacity"] * (np.float32(1) - m["transmission"])),
        V.TEXCOORD0: lambda: np.array([*fract(uv[0:2]), 0], np.float32),
        V.TEXCOORD1: lambda: np.array([*fract(uv[2:4]), 0], np.float32),
        V.TRIANGLE_ID: lambda: _hash_to_color((np.uint64(np.uint32(rprim & 0xFFFFFFFF)) * np.uint64(65537) + np.uint64(np.uint32(prim & 0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)),
        V.FACE_ORIENTATION: lambda: np.array([0, 1, 0] if front else [1, 0, 0], np.float32),
        V.OCCLUSION: lambda: s3(m["occlusion"]),
        V.CLEARCOAT_FACTOR: lambda: s3(m["clearcoat"]),
        V.CLEARCOAT_ROUGHNESS: lambda: s3(m["clearcoatRoughness"]),
        V.CLEARCOAT_NORMAL: lambda: m["Nc"] * half + half,
        V.SHEEN_COLOR: lambda: m["sheenColor"],
        V.SHEEN_ROUGHNESS: lambda: s3(m["sheenRoughness"]),
        V.SPECULAR_FACTOR: lambda: s3(m["specular"]),
        V.SPECULAR_COLOR: lambda: m["specularColor"],
        V.TRANSMISSION_FACTOR: lambda: s3(m["transmission"]),
        V.IRIDESCENCE_FACTOR: lambda: s3(m["iridescence"]),
        V.IRIDESCENCE_THICKNESS: lambda: s3(m["iridescenceThickness"] / np.float32(1200)),
        V.ANISOTROPY_STRENGTH: lambda: s3(np.sqrt(np.clip((r[0] - r[1]) / np.maximum(np.float32(1) - r[1], np.float32(1e-5)), 0, 1)).astype(np.float32)),
        V.DIFFUSE_TRANSMISSION_FACTOR: lambda: s3(m["diffuseTransmissionFactor"]),
        V.DIFFUSE_TRANSMISSION_COLOR: lambda: m["diffuseTransmissionColor"],
    }
    if mode == V.CLAY:
        return MATERIAL_OVERRIDE, None
    if mode == V.OPACITY_MICROMAP:
        if omm < 0:
            return RENDERED, None
        return COLOR_OVERRIDE, np.array([0.90, 0.80, 0.10] if omm > 0 else [0.15, 0.75, 0.15], np.float32)
    if mode in table:
        return COLOR_OVERRIDE, np.asarray(table[mode](), np.float32)
    return RENDERED, None


def test_enum_matches_reference_order():
    assert len(V) == MI_VIZ_COUNT == 30 and [int(v) for v in V] == list(range(30))
    assert V.CLAY == 12 and V.TRIANGLE_ID == 13 and V.OPACITY_MICROMAP == 29


def test_hash_to_color_bit_exact(viz):
    rng = np.random.default_rng(7)
    ids = [0, 1, 65537, 0xFFFFFFFF, *rng.integers(0, 2 ** 32, 2000, dtype=np.uint64).tolist()]
    out = (F * 3)()
    for i in ids:
        viz.dev_hash_to_color(C.c_uint32(int(i)), out)
        np.testing.assert_array_equal(np.array(out[:], np.float32), _hash_to_color(int(i)), err_msg=str(i))


MODES = list(range(0, 31)) + [-1, 31, 1000]


@pytest.mark.parametrize("mode", MODES)
def test_apply_visualization_matches_numpy(viz, mode):
    rng = np.random.default_rng(1000 + (mode & 0xFFFF))
    colour = (F * 3)()
    for k in range(200):
        m, arr = _material(viz, rng)
        uv = rng.uniform(-3.0, 3.0, 4).astype(np.float32)
        front = bool(rng.integers(0, 2))
        rprim, prim = int(rng.integers(-1, 5000)), int(rng.integers(-1, 1 << 20))
        omm = int(rng.integers(-1, 2))
        before = arr.copy()
        buf = (F * len(arr))(*arr.tolist())
        res = viz.dev_apply_visualization(buf, (F * 4)(*uv.tolist()), int(front), mode, rprim, prim, omm, colour)
        after = np.array(buf[:], np.float32)
        want_res, want = expected(mode, m, uv, front, rprim, prim, omm)
        assert res == want_res, (mode, k, res, want_res)
        got = np.array(colour[:], np.float32)
        if want_res == COLOR_OVERRIDE:
            if mode == V.TRIANGLE_ID:
                np.testing.assert_array_equal(got, want)
            else:
                np.testing.assert_array_max_ulp(got, want, maxulp=4)
            np.testing.assert_array_equal(after, before)  # a colour view leaves the material alone
        elif want_res == MATERIAL_OVERRIDE:
            # clay: base colour (0.8, 0.75, 0.7), metallic 0, roughness 0.5 squared, no emission; every other field kept
            exp = before.copy()
            for name, val in (("baseColor", [0.8, 0.75, 0.7]), ("metallic", [0.0]), ("roughness", [0.25, 0.25]), ("emissive", [0.0, 0.0, 0.0])):
                o, n = viz.offsets[name]
                exp[o:o + n] = np.array(val, np.float32)
            np.testing.assert_array_equal(after, exp)
        else:  # "rendered": nothing touched
            np.testing.assert_array_equal(after, before)
