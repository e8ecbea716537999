"""Child process of tests/test_gpu_api_state.py::test_read_backs_equal_the_bound_tensors: the whole-image read-backs against torch tensors bound
as the accumulator and the guide images, and against the raw accumulator pointer.  torch is imported BEFORE libmi_pt.so is loaded, so that both
use the one HIP runtime torch brings.
usage: python tests/api_state_device_child.py"""
import ctypes as C
import os
import sys

import torch  # (first: see above)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import parity_util as pu  # noqa: E402
from vk_gltf_renderer_amd import _capi as capi  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402

W, H, TILE = 40, 24, 16  # (as in tests/test_gpu_api_state.py)
PX = W * H


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1))


def main():
    assert torch.cuda.is_available()
    st = pu.Setup(os.path.join(ROOT, "assets", "Box.glb"), W, H, max_depth=3)
    tr = ptmod.PathTracer(st.scene)
    lib = tr._l
    tr.set_tile_partition(0, 1, TILE)
    tr.resize(W, H)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    albedo, normal = torch.zeros_like(accum), torch.zeros_like(accum)
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tr.bind_accum(accum.data_ptr())
    tr.bind_guides(albedo.data_ptr(), normal.data_ptr(), depth.data_ptr())
    p = st.frame_params(0, 0)
    p.flags |= capi.MI_PT_USE_OPTIX_DENOISER
    tr.render_frame(p)
    got = tr.read_accum()  # (synchronises the device)
    assert np.isfinite(got).all() and np.abs(got[..., :3]).sum() > 0
    assert same(got, accum.cpu().numpy())
    a, n = tr.read_guides()
    assert np.abs(a).sum() > 0 and np.abs(n).sum() > 0
    assert same(a, albedo.cpu().numpy()) and same(n, normal.cpu().numpy())
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    only_a, only_n = np.full((H, W, 4), -7.0, np.float32), np.full((H, W, 4), -7.0, np.float32)
    assert lib.mi_pt_read_guides(tr._p, fp(only_a), None) == 0 and same(only_a, a)
    assert lib.mi_pt_read_guides(tr._p, None, fp(only_n)) == 0 and same(only_n, n)
    d = tr.read_depth()
    assert same(d, depth.cpu().numpy()) and (d != 0).any()
    # unbound: the instance's own accumulator, read through its device pointer with the HIP runtime this process has loaded
    tr.bind_accum(0)
    tr.bind_guides(0, 0, 0)
    tr.render_frame(st.frame_params(0, 0))
    own = tr.read_accum()
    ptr = lib.mi_pt_accum_device_ptr(tr._p)
    assert ptr and ptr != accum.data_ptr()
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    via = np.zeros((H, W, 4), np.float32)
    assert hip.hipMemcpy(via.ctypes.data, ptr, PX * 16, 2) == 0  # hipMemcpyDeviceToHost
    assert same(own, via) and np.abs(own[..., :3]).sum() > 0
    tr.close()
    print("API_STATE_DEVICE_OK")


if __name__ == "__main__":
    main()
