"""The closest-hit walk with its triangle fetch overlapped with the node step (TriRound, pt_kernels.hip; LaneStack2::pop, pt_bvh8.h) computes what
it computed: nothing changed in what is tested, for which ray, or in which order the owners collect, so its images are those of the BVH2 walk --
which has no rounds and no group stack -- bit for bit.

  * Atrium class scene with alpha foliage, one wave of rays and more (64 x 32, depth 4): rounds of 20 and more owners, the per-lane cap, deferred
    alpha tests; with 1 and with 64 frames in flight.
  * The stack's LDS-to-scratch boundary.  A scene that provably sends rays beyond 12 stack groups could not be had: the tree is built on the device
    and nothing reads it back, so the depth a nested-cluster scene reaches cannot be confirmed on the host (LABNOTES.md).  The boundary is covered
    at function level instead (tests/device_kat/kat_lane_stack.hip): every lane of a wave pushes and pops at a depth of its own, 0 .. 20, with a
    global load in flight across the pops, and every popped group, the loaded word and the final stack pointer are compared with a list in Python."""
import ctypes as C

import numpy as np
import pytest

import device_kat_lib as kat
import parity_util as pu
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu

MAX_DEPTH = 20                  # KAT_STACK_MAX_DEPTH
OUT_WORDS = 4 * MAX_DEPTH + 2   # KAT_STACK_OUT_WORDS
LDS_GROUPS = 12                 # BVH8_STACK_LDS


@pytest.fixture(scope="module")
def atrium(built, tmp_path_factory):
    path = scenegen.scene_atrium_class(str(tmp_path_factory.mktemp("walk_overlap") / "atrium.glb"), detail=0.1, tex_size=64)
    s = pu.Setup(path, 64, 32, max_depth=4)
    return s, pu.render_gpu(s, 2, bvh=1)  # the reference: rendered once, shared, left alone


@pytest.mark.parametrize("in_flight", [1, 64])
def test_images_are_those_of_the_bvh2_walk(atrium, in_flight):
    s, ref = atrium
    wide = pu.render_gpu(s, 2, bvh=0, in_flight=in_flight)
    assert np.isfinite(wide["accum"]).all() and wide["accum"][..., :3].max() > 0.0
    assert (wide["accum"] == ref["accum"]).all()
    assert (wide["selection"] == ref["selection"]).all() and (wide["depth"] == ref["depth"]).all()
    for k in ("segments", "shadowRays", "textureTaps"):
        assert wide["stats"][k] == ref["stats"][k], k
    assert wide["stats"]["trisClosest"] > 0 and wide["stats"]["nodesClosest"] < ref["stats"]["nodesClosest"]  # (the 8-wide walk did run)


def _group(case, lane, level):
    base = (0x01000193 * (case + 1) + 0x10000 * lane + level) & 0xffffffff
    return base, (~base ^ (level << 24)) & 0xffffffff


def _expected(depths, probe):
    out = np.full((len(depths), 64, OUT_WORDS), 0xffffffff, np.uint32)
    for c in range(len(depths)):
        for lane in range(64):
            d = int(depths[c, lane])
            for p, (n, tag) in enumerate(((d, 0), (MAX_DEPTH - d, 100))):
                stack = [_group(c, lane, i + tag) for i in range(n)]
                for i in range(n):
                    out[c, lane, (p * MAX_DEPTH + i) * 2:(p * MAX_DEPTH + i) * 2 + 2] = stack.pop()
            out[c, lane, 4 * MAX_DEPTH] = probe[c, lane]
            out[c, lane, 4 * MAX_DEPTH + 1] = 0
    return out


def test_lane_stack_across_the_lds_scratch_boundary():
    lanes = np.arange(64)
    rng = np.random.default_rng(1234)
    depths = np.stack([lanes % (MAX_DEPTH + 1),                         # every depth 0 .. 20 side by side in one wave
                       np.full(64, LDS_GROUPS),                         # LDS exactly full: no lane in scratch
                       np.where(lanes % 2 == 0, LDS_GROUPS + 1, LDS_GROUPS),  # half of the wave one group beyond
                       np.where(lanes == 37, MAX_DEPTH, 3),             # one deep lane among shallow ones
                       np.full(64, MAX_DEPTH), np.zeros(64, np.int64),
                       rng.integers(0, MAX_DEPTH + 1, 64), rng.integers(LDS_GROUPS - 2, LDS_GROUPS + 3, 64)]).astype(np.int32)
    probe = rng.integers(0, 2 ** 32, depths.shape, dtype=np.uint64).astype(np.uint32)
    out = np.zeros((len(depths), 64, OUT_WORDS), np.uint32)
    fn = kat.lib().kat_lane_stack
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    depths, probe = np.ascontiguousarray(depths), np.ascontiguousarray(probe)
    err = fn(len(depths), depths.ctypes.data_as(C.c_void_p), probe.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert err == 0, "kat_lane_stack: hipError_t %d" % err
    want = _expected(depths, probe)
    bad = np.argwhere(out != want)
    assert len(bad) == 0, (len(bad), bad[:8].tolist(), [hex(int(out[tuple(b)])) for b in bad[:8]], [hex(int(want[tuple(b)])) for b in bad[:8]])
