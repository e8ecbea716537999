"""Shared by the environment-update tests (tests/test_env_update_on_host.py, tests/test_gpu_env_update.py and its child): the input maps, the
validity check of an alias table in float64, the comparison with the host route (mi_hdr_from_pixels), the host shim and the golden file.

The inputs come from an integer hash written out below, not from numpy's generators: tests/golden/env_update_cases.npz holds tables made from
them, so they must be the same floats under every numpy.

The bounds of `check_table` are derived, not measured.  A table entry's only error is the float32 rounding of q <= 1, at most 2^-25; it
enters two texels (the slot's own and its alias).  The test's own float32 importance may differ from the library's by one rounding, 2^-24
relative (numpy's cosine against the C library's in the row area).  So, with p = mass / n and p_true = importance / total in float64:
    sum |p - p_true| <= 2^-23        |p_i - p_true_i| <= (1 + k_i) 2^-25 / n + 2^-23 p_true_i + 1e-12,   k_i = slots that alias to i."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (run as a script, to rewrite the golden file)
    sys.path.insert(0, ROOT)

from vk_gltf_renderer_amd import _capi as capi  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "env_update_cases.npz")
HDR = os.path.join(ROOT, "assets", "std_env.hdr")
# (width, height): one texel; one row; odd and tiny; exactly two 1024-texel scan tiles; a partial third tile, prefixes that cross tiles
SMALL_SIZES = ((1, 1), (2, 1), (5, 3), (64, 32), (65, 33))
PATTERNS = ("tail", "constant", "black", "onehot", "halves")
SMALL_CASES = tuple((w, h, p) for (w, h) in SMALL_SIZES for p in PATTERNS)
UNIFORM_PDF = np.float32(1.0 / (4.0 * np.pi))
ACCEL_DTYPE = np.dtype([("alias", "<u4"), ("q", "<f4")])


def case_id(case):
    return "%dx%d-%s" % case


def _hash01(count, seed):
    """count floats in [0, 1) with 24 random bits each: splitmix64 of the counter."""
    with np.errstate(over="ignore"):
        z = (np.arange(count, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x632BE59BD9B4E019)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float32) / np.float32(1 << 24)).astype(np.float32)


def make_pixels(width, height, pattern):
    """The H x W x 3 float32 map of a case."""
    n = width * height
    if pattern == "constant":
        return np.full((height, width, 3), 0.25, np.float32)
    if pattern == "black":
        return np.zeros((height, width, 3), np.float32)
    if pattern == "onehot":  # one heavy texel serves n - 1 lights
        px = np.zeros((height, width, 3), np.float32)
        px[height // 2, width // 3] = (1.0, 3.0, 2.0)
        return px
    if pattern == "halves":  # bright rows over dim ones: a long run of consecutive heavies, each chaining to the next
        px = np.full((height, width, 3), 0.01, np.float32)
        px[:max(1, height // 2)] = 5.0
        return px
    assert pattern == "tail"
    seed = width * 1000 + height
    u = _hash01(n, seed)
    u2 = u * u
    u4 = u2 * u2
    m = (u4 * u4).astype(np.float32)  # u^8 by exact float32 squarings: most of the mass in a few texels
    m[_hash01(n, seed + 1) < np.float32(0.3)] = 0.0  # 30 % black
    m = m.reshape(height, width)
    if n > 1:
        m[height // 3, width // 2] = 6.0e4
    tint = (np.float32(0.25) + np.float32(0.75) * _hash01(3 * n, seed + 2)).reshape(height, width, 3)  # (the brightest channel varies)
    return (m[..., None] * tint).astype(np.float32)


def gradient_with_patch(width=64, height=32):
    """The convergence test's map: a smooth gradient and a 4 x 4 patch of value 50."""
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    px = np.stack([0.2 + 0.6 * x / width, 0.3 + 0.4 * y / height, 0.8 - 0.5 * x / width], -1).astype(np.float32)
    px[height // 4:height // 4 + 4, width // 2:width // 2 + 4] = 50.0
    return px


def load_hdr_pixels():
    """assets/std_env.hdr as the loader decodes it: (750, 1500, 3) float32."""
    h = capi.host_lib()
    p = C.c_void_p()
    assert h.mi_hdr_load(HDR.encode(), C.byref(p)) == 0
    try:
        e = h.mi_hdr_env(p).contents
        rgba = np.ctypeslib.as_array(e.rgba, shape=(e.height, e.width, 4))
        return np.ascontiguousarray(rgba[..., :3])
    finally:
        h.mi_hdr_destroy(p)


def host_route(pixels):
    """What the parent's route makes of the map (mi_hdr_from_pixels): rgba, alias, q, integral."""
    h = capi.host_lib()
    px = np.ascontiguousarray(pixels[..., :3], np.float32)
    p = C.c_void_p()
    assert h.mi_hdr_from_pixels(px.shape[1], px.shape[0], px.ctypes.data_as(C.POINTER(C.c_float)), C.byref(p)) == 0
    try:
        e = h.mi_hdr_env(p).contents
        n = e.width * e.height
        rgba = np.ctypeslib.as_array(e.rgba, shape=(e.height, e.width, 4)).copy()
        accel = np.frombuffer(C.string_at(e.accel, n * 8), ACCEL_DTYPE).reshape(e.height, e.width)
        return rgba, accel["alias"].copy(), accel["q"].copy(), float(e.integral)
    finally:
        h.mi_hdr_destroy(p)


def row_areas(width, height):
    theta = np.arange(height, dtype=np.float64) * (np.pi / height)
    return (np.cos(theta) - np.cos(theta + np.pi / height)) * (2.0 * np.pi / width)


def importance(pixels):
    """float32 importances of a map, as float64, and their total."""
    h, w = pixels.shape[:2]
    m = pixels[..., :3].max(-1).astype(np.float64)
    imp = (row_areas(w, h)[:, None] * m).astype(np.float32).astype(np.float64).reshape(-1)
    return imp, float(imp.sum())


def ulps(a, b):
    """Distance of non-negative float32 values in units of the last place."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def check_table(pixels, rgba, alias, q, integral):
    """The normative contract of a resident environment, in float64 on what read_environment returned.  Returns the figures it asserted on."""
    h, w = pixels.shape[:2]
    n = w * h
    assert rgba.shape == (h, w, 4) and alias.shape == (h, w) and q.shape == (h, w)
    assert rgba[..., :3].tobytes() == np.ascontiguousarray(pixels[..., :3]).tobytes()  # rgb: the caller's values
    alias, qd = alias.reshape(-1).astype(np.int64), q.reshape(-1).astype(np.float64)
    assert (alias >= 0).all() and (alias < n).all() and (qd >= 0.0).all() and (qd <= 1.0).all()
    imp, total = importance(pixels)
    if total <= 0.0:
        assert (alias == np.arange(n)).all() and (q == 1.0).all() and integral == 0.0
        assert (rgba[..., 3] == UNIFORM_PDF).all()
        return {"l1": 0.0, "worst": 0.0}
    mass = qd + np.bincount(alias, weights=1.0 - qd, minlength=n)
    p, p_true = mass / n, imp / total
    k = np.bincount(alias, minlength=n)
    err = np.abs(p - p_true)
    bound = (1 + k) * 2.0 ** -25 / n + 2.0 ** -23 * p_true + 1e-12
    l1, worst = float(err.sum()), float((err / bound).max())
    print("env table %dx%d: L1 %.3e (bound %.3e), worst per-texel error / bound %.3f, max fan-in %d" % (w, h, l1, 2.0 ** -23, worst, int(k.max())))
    assert l1 <= 2.0 ** -23, l1
    assert (err <= bound).all(), worst
    return {"l1": l1, "worst": worst}


def check_against_host_route(pixels, rgba, integral):
    """rgb bit for bit, integral within 1 float ulp, alpha within 2 (the two double totals differ by far less than a float ulp, so
    float(1 / total) differs by at most one rounding, and one product follows it); the black map: 1 / (4 pi) exactly."""
    h_rgba, _, _, h_integral = host_route(pixels)
    assert rgba[..., :3].tobytes() == h_rgba[..., :3].tobytes()
    assert ulps(np.float32(integral), np.float32(h_integral)) <= 1, (integral, h_integral)
    assert int(ulps(rgba[..., 3], h_rgba[..., 3]).max()) <= 2
    if h_integral == 0.0:
        assert rgba[..., 3].tobytes() == h_rgba[..., 3].tobytes() and integral == 0.0


def make_environment(rgba, alias, q, integral):
    """A capi.MiPtEnvironment over read-back tables (for mi_pt_set_environment), and what keeps its memory alive."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    accel = np.empty(alias.shape, ACCEL_DTYPE)
    accel["alias"], accel["q"] = alias, q
    e = capi.MiPtEnvironment()
    e.rgba = rgba.ctypes.data_as(C.POINTER(C.c_float))
    e.accel = C.cast(accel.ctypes.data, C.POINTER(capi.MiEnvAccel))
    e.width, e.height, e.integral = rgba.shape[1], rgba.shape[0], integral
    return e, (rgba, accel)


# ---- the host shim (tests/host_shim/env_update_on_host.cpp)
def build_shim(out_dir):
    out = os.path.join(str(out_dir), "libenv_update_on_host.so")
    d = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-I" + d, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"), "-o", out, os.path.join(d, "env_update_on_host.cpp")], check=True)
    L = C.CDLL(out)
    L.dev_env_update.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dev_env_update.restype = C.c_int
    L.dev_env_scratch_bytes.argtypes = [C.c_int, C.c_int]
    L.dev_env_scratch_bytes.restype = C.c_uint64
    return L


def shim_update(L, pixels):
    """The passes of pt_env_update.h on the host: (rgba, alias, q, integral, info)."""
    px = np.ascontiguousarray(pixels, np.float32)
    h, w, ch = px.shape
    rgba = np.full((h, w, 4), np.nan, np.float32)
    accel = np.zeros((h, w), ACCEL_DTYPE)
    accel["alias"] = 0xFFFFFFFF
    info = np.zeros(6, np.float64)
    tiles = L.dev_env_update(w, h, ch, px.ctypes.data, rgba.ctypes.data, accel.ctypes.data, info.ctypes.data)
    assert tiles == (w * h + 1023) // 1024
    names = ("total", "scale", "totalDeficit", "invTotal", "lightTexels", "texelsSanitised")
    return rgba, accel["alias"].copy(), accel["q"].copy(), float(np.float32(info[0])), dict(zip(names, info.tolist()))


def golden_arrays(L):
    """What tests/golden/env_update_cases.npz holds: alias, q, alpha and integral of every small case, from the shim."""
    out = {}
    for case in SMALL_CASES:
        rgba, alias, q, integral, _ = shim_update(L, make_pixels(*case))
        name = case_id(case)
        out[name + "/alias"], out[name + "/q"] = alias, q
        out[name + "/alpha"], out[name + "/integral"] = np.ascontiguousarray(rgba[..., 3]), np.float32(integral)
    return out


def same_as_golden(golden, case, rgba, alias, q, integral):
    name = case_id(case)
    return {k: bool(np.asarray(v).tobytes() == golden[name + "/" + k].tobytes())
            for k, v in (("alias", alias), ("q", q), ("alpha", np.ascontiguousarray(rgba[..., 3])), ("integral", np.float32(integral)))}


if __name__ == "__main__":  # python tests/env_update_util.py <scratch directory>: rewrites the golden file from the shim
    np.savez_compressed(GOLDEN, **golden_arrays(build_shim(sys.argv[1])))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
