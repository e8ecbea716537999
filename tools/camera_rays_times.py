"""Cost of caller-supplied camera rays on the bench's atrium workload (1920 x 1080, depth 12), from mi_pt_enable_timing: k_generate_rays against
k_generate on one MI_PT_NO_PACKET=1 instance, and the whole batch in three configurations -- exported rays bound, built-in camera with
MI_PT_NO_PACKET=1, built-in camera by default (the fused packet kernel).  8 and 64 frames in flight; the rays are bound in device memory.
usage: python tools/camera_rays_times.py [--batches N] [--out FILE]     (needs a GPU; torch is imported first: one HIP runtime)"""
import argparse
import os
import sys

import torch  # noqa: F401  (before libmi_pt.so)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bench  # noqa: E402
from vk_gltf_renderer_amd import _capi as capi  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402


def tracer(scene, fi, sky, w, h, no_packet):
    old = os.environ.get("MI_PT_NO_PACKET")
    if no_packet:
        os.environ["MI_PT_NO_PACKET"] = "1"
    else:
        os.environ.pop("MI_PT_NO_PACKET", None)
    try:
        tr = ptmod.PathTracer(scene)
    finally:
        if old is None:
            os.environ.pop("MI_PT_NO_PACKET", None)
        else:
            os.environ["MI_PT_NO_PACKET"] = old
    tr.resize(w, h)
    tr.set_frame_info(fi)
    tr.set_sky(sky)
    return tr


def timed(tr, params, n, batches):
    """ms per batch of n frames: (generate, whole batch), after one first-frame batch and one more to warm up"""
    def batch(k):
        params.frameCount, params.totalSamples = k * n, k * n
        params.flags = capi.MI_PT_FIRST_FRAME if k == 0 else 0
        tr.render_frames(params, n)
    batch(0)
    batch(1)
    tr.synchronize()
    tr.enable_timing(True)
    for k in range(2, 2 + batches):
        batch(k)
    t = tr.frame_timing()
    tr.enable_timing(False)
    return t["generateMs"] / batches, t["totalMs"] / batches, t["tracePrimaryLaunches"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = bench.WORKLOADS["atrium"]
    W, H = w["width"], w["height"]
    scene = ptmod.Scene(bench.scene_path("atrium", 0))
    scene.cut_alpha(bench.ALPHA_CUT_DEFAULT)
    fi, angle, focal = ptmod.camera_frame_info(scene.camera(0), W, H)
    sky = ptmod.default_sky()
    params = ptmod.default_params()
    params.maxDepth, params.numSamples, params.pixelAngle, params.focalDistance = w["depth"], 1, angle, focal
    lines = ["caller-supplied camera rays, atrium %d x %d depth %d, %d timed batches per figure (ms per batch)" % (W, H, w["depth"], args.batches)]
    for n in (8, 64):
        np_ = tracer(scene, fi, sky, W, H, True)
        g0, b0, _ = timed(np_, params, n, args.batches)
        params.frameCount = 0
        rays = np_.make_camera_rays(params, n, device=True)
        np_.set_camera_rays(rays, unit=True)
        g1, b1, launches = timed(np_, params, n, args.batches)
        assert launches == 0
        np_.close()
        del rays
        torch.cuda.empty_cache()
        df = tracer(scene, fi, sky, W, H, False)
        _, b2, launches = timed(df, params, n, args.batches)
        assert launches > 0
        df.close()
        lines.append("frames in flight %2d: k_generate_rays %.3f  k_generate %.3f | batch: bound exported rays %.2f  built-in MI_PT_NO_PACKET=1 %.2f  built-in default %.2f"
                     % (n, g1, g0, b1, b0, b2))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
