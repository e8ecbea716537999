"""Child process of tests/test_gpu_camera_rays.py::test_device_forms_with_torch_tensors: the device forms of the camera-ray entry points
(mi_pt_set_camera_rays_device, mi_pt_make_camera_rays_device) fed with torch tensors.  torch is imported BEFORE libmi_pt.so is loaded, so that
both use the one HIP runtime torch brings.
usage: python tests/camera_rays_device_child.py <scratch directory>"""
import os
import sys

import torch  # (first: see above)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import parity_util as pu  # noqa: E402
from vk_gltf_renderer_amd import _capi as capi  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402

W, H = 72, 40


def params(st, start, first):
    p = st.frame_params(start, start)
    p.flags = capi.MI_PT_FIRST_FRAME if first else 0
    return p


def render(tr, st, n):
    tr.render_frames(params(st, 0, True), n)
    tr.render_frames(params(st, n, False), n)
    return tr.read_accum(), tr.read_selection(), tr.read_depth()


def main(tmp):
    assert torch.cuda.is_available()
    glb = scenegen.scene_animated(os.path.join(tmp, "animated.glb"))
    st = pu.Setup(glb, W, H, max_depth=4, params_edit=lambda p: setattr(p, "aperture", 0.05))
    for bvh in (0, 1):
        tr = ptmod.PathTracer(st.scene, bvh=bvh)
        tr.resize(W, H)
        tr.set_frame_info(st.frame_info)
        tr.set_sky(st.sky)
        for n in (3, 64):
            host = tr.make_camera_rays(params(st, 0, True), 2 * n)
            m0 = tr.memory()
            dev = tr.make_camera_rays(params(st, 0, True), 2 * n, device=True)
            assert dev.is_cuda and tuple(dev.shape) == (2 * n, H, W, 8) and dev.dtype == torch.float32
            assert dev.cpu().numpy().tobytes() == host.tobytes(), (bvh, n)  # the two forms of make: the same bytes
            tr.set_camera_rays(dev, unit=True)
            m1 = tr.memory()
            assert all(m1[k] == m0[k] for k in ("sceneBytes", "rendererBytes", "pathStateBytes")), (m0, m1)  # the device forms allocate nothing
            on_device = render(tr, st, n)
            m2 = tr.memory()  # (the path arrays have grown to n frames in flight meanwhile)
            tr.set_camera_rays(host, unit=True)
            assert tr.memory()["rendererBytes"] - m2["rendererBytes"] == 2 * n * W * H * 32
            on_host = render(tr, st, n)
            for a, b in zip(on_device, on_host):
                assert a.tobytes() == b.tobytes(), (bvh, n)
            assert np.isfinite(on_host[0]).all() and (on_host[1] != 0).sum() > 100
            tr.set_camera_rays(None)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # (the binding takes torch's current stream)
            on_side = tr.make_camera_rays(params(st, 0, True), 2, device=True)
        side.synchronize()
        assert on_side.cpu().numpy().tobytes() == tr.make_camera_rays(params(st, 0, True), 2).tobytes()
        for bad in (torch.zeros((H, W, 7), device="cuda"), torch.zeros((H, W + 1, 8), device="cuda"), torch.zeros((H, W, 8), device="cuda").double()):
            try:
                tr.set_camera_rays(bad)
                raise SystemExit("a tensor of the wrong shape or type was accepted")
            except ValueError:
                pass
        tr.close()
    print("CAMERA_RAYS_DEVICE_OK")


if __name__ == "__main__":
    main(sys.argv[1])
