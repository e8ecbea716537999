"""Cost of the motion vectors and the temporal pass (LABNOTES.md, "Temporal reprojection"), on scenegen.scene_atrium_class at --size.

Three measurements, each the median of --repeats timed with HIP events after --warmup, A and B alternating in one process and an A/A pair
for the spread:
  1. an 8-frame MI_PT_FIRST_FRAME batch with mi_pt_set_temporal off (A, A') against on (B): what the motion kernel and the snapshot add;
  2. mi_pt_denoise_svgf (A, A') against mi_pt_denoise_temporal (B) at equal a-trous iterations;
  3. mi_pt_denoise_temporal with 0 iterations (k_svgf_reproject + the re-modulation) as a share of 8 TB/s, the bytes counted from the record
     sizes: reproject 68 B in + 64 B out per pixel (its four taps of 48 B are shared between neighbours and counted as L2 traffic), the
     re-modulation 48 B in + 16 B out.
Nothing here is a threshold.  Prints one JSON line.

usage: python tools/temporal_bench.py [--size 1920 1080] [--repeats 20] [--warmup 3] [--iterations 5]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import parity_util as pu  # noqa: E402
from vk_gltf_renderer_amd import _capi as capi  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402


def timed(call):
    """device milliseconds of `call` on the default stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(calls, repeats, warmup):
    """medians of the named calls, run round-robin"""
    times = {k: [] for k in calls}
    for r in range(warmup + repeats):
        for k, call in calls.items():
            t = timed(call)
            if r >= warmup:
                times[k].append(t)
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=5)
    a = ap.parse_args()
    w, h = a.size
    torch.cuda.init()
    with tempfile.TemporaryDirectory() as tmp:
        glb = scenegen.scene_atrium_class(os.path.join(tmp, "atrium.glb"))
        st = pu.Setup(glb, w, h, max_depth=5, params_edit=lambda p: setattr(p, "flags", p.flags | capi.MI_PT_USE_OPTIX_DENOISER))
        tracers = {}
        for name, temporal in (("off", False), ("off_again", False), ("on", True)):
            tr = ptmod.PathTracer(st.scene)
            tr.resize(w, h)
            tr.set_frame_info(st.frame_info)
            tr.set_sky(st.sky)
            tr.set_temporal(temporal)
            tracers[name] = tr
        first = st.frame_params(0, 0)
        res = {"scene": "scene_atrium_class", "triangles": st.scene.num_triangles, "size": [w, h], "repeats": a.repeats}
        res["first_frame_batch_of_8_ms"] = alternate({k: (lambda tr=tr: tr.render_frames(first, 8)) for k, tr in tracers.items()}, a.repeats, a.warmup)
        on = tracers["on"]
        it = a.iterations
        tp, tp0 = on.default_temporal(iterations=it), on.default_temporal(iterations=0)
        svgf = lambda tr: (lambda: tr.denoise_svgf(iterations=it, read=False))  # noqa: E731
        res["denoise_ms"] = alternate({"svgf": svgf(tracers["off"]), "svgf_again": svgf(tracers["off_again"]), "temporal": lambda: on.denoise_temporal(tp, read=False),
                                       "temporal_0_iterations": lambda: on.denoise_temporal(tp0, read=False)}, a.repeats, a.warmup)
        nbytes = w * h * (68 + 64 + 48 + 16)
        res["temporal_stage_bytes"] = nbytes
        res["temporal_stage_share_of_8TBs"] = round(nbytes / (res["denoise_ms"]["temporal_0_iterations"] * 1e-3) / 8e12, 4)
        res["memory_bytes_temporal"] = on.memory()["rendererBytes"] - tracers["off"].memory()["rendererBytes"]
        for tr in tracers.values():
            tr.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
