"""Child process of tests/test_gpu_image_passes.py: every case of tests/image_pass_cases.py through mi_pt_denoise, mi_pt_denoise_svgf or
mi_pt_denoise_temporal on images this process puts in front of them.  The accumulator and the guide images are torch tensors bound with
mi_pt_bind_accum / mi_pt_bind_guides; torch is imported BEFORE libmi_pt.so is loaded, so that both use the one HIP runtime torch brings.
The results go to an .npz; the parent does the comparing.
usage: python tests/image_pass_device_child.py OUT.npz"""
import os
import sys

import torch  # (first: see above)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import image_pass_cases as ipc  # noqa: E402
import parity_util as pu  # noqa: E402
from vk_gltf_renderer_amd import _capi as capi  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402


def run_size(W, H, cases, results):
    st = pu.Setup(os.path.join(ROOT, "assets", "Box.glb"), W, H, max_depth=3)
    tr = ptmod.PathTracer(st.scene)
    try:
        tr.resize(W, H)
        tr.set_frame_info(st.frame_info)
        tr.set_sky(st.sky)
        accum = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        albedo, normal = torch.zeros_like(accum), torch.zeros_like(accum)
        depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        tr.bind_accum(accum.data_ptr())
        tr.bind_guides(albedo.data_ptr(), normal.data_ptr(), depth.data_ptr())
        for c in sorted(cases, key=lambda c: c.kind == "temporal"):  # (the temporal cases last: mi_pt_set_temporal stays on)
            if c.kind == "temporal" and not tr.temporal:
                tr.set_temporal(True)
            if c.frames > 1:  # the moment covers the frames only when they were rendered, with the guides on
                total = 0
                for f in range(c.frames):
                    p = st.frame_params(f, total)
                    p.flags |= capi.MI_PT_USE_OPTIX_DENOISER
                    tr.render_frame(p)
                    total += p.numSamples
                tr.synchronize()
            albedo.copy_(torch.from_numpy(c.albedo))
            normal.copy_(torch.from_numpy(c.normal))
            depth.copy_(torch.from_numpy(c.depth))
            if c.frames > 1 and not c.rewrite:
                accum.copy_(torch.from_numpy(c.color))
            torch.cuda.synchronize()
            if c.frames == 1 or c.rewrite:
                tr.write_accum(c.color)  # (into the bound tensor)
            if c.kind == "atrous":
                out = tr.denoise(c.iterations, *c.sigmas)
            elif c.kind == "svgf":
                out = tr.denoise_svgf(c.iterations, *c.sigmas)
            else:
                tr.reset_history()
                out = tr.denoise_temporal(iterations=c.iterations, sigmaLuminance=c.sigmas[0], sigmaNormal=c.sigmas[1], sigmaDepth=c.sigmas[2])
                results[c.name + "/first_hit"] = tr.read_first_hit()
            assert np.array_equal(accum.cpu().numpy(), c.color), c.name  # the denoisers leave their input alone
            results[c.name] = out
    finally:
        tr.close()


def main():
    assert torch.cuda.is_available()
    results = {}
    for (W, H) in ipc.SIZES:
        run_size(W, H, [c for c in ipc.all_cases() if (c.W, c.H) == (W, H)], results)
    np.savez(sys.argv[1], **results)
    print("IMAGE_PASS_DEVICE_OK", len(results))


if __name__ == "__main__":
    main()
