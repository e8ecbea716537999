"""Rate of the ray queries (mi_pt_query_rays_device, csrc/device/query.hip) on the atrium-class scene at bench detail (LABNOTES.md, "Ray
queries and picking"): 2 M coherent rays -- the camera rays of a 1920 x 1080 frame in image order, the rays mi_pt_pick forms for the pixel
centres -- and 2 M incoherent rays of the recipe of tests/query_util.py (origins on a sphere around the scene and inside its bounds, aimed at
uniform points of the bounds), in CLOSEST and ANY mode.  Device form, timed with events on the stream around 20 back-to-back launches, best of
five such windows after a warm-up launch.  For scale: the segments per second of k_trace_closest (every bounce's closest-hit launch, the camera rays' packet walk
included) over a few frames of the same scene, from mi_pt_get_frame_timing and the segment counter.  mi_pt_pick itself (host form: upload, kernel,
read-back of 64 B per pixel) is timed by the wall clock next to it.  Prints one JSON line.  Not a test; run it under `timeout`.

--alpha / --cull / --max-hits add a row per ray set for the _ex entry point under those options (closest hit, or NEAREST_K when --max-hits > 1).

usage: timeout 600 python tools/query_bench.py [--detail 0.8] [--size 1920 1080] [--rays 2073600] [--bvh 0] [--sliver] [--alpha cutoff] [--cull material]
       [--max-hits 4]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402  (before libmi_pt.so is loaded: both then use the one HIP runtime torch brings)
import numpy as np  # noqa: E402

import parity_util as pu  # noqa: E402
import query_util as qu  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402


def camera_rays(fi, width, height):
    """The rays of the pixel centres in image order (getRay of csrc/device/pt_camera.h in float64, rounded: a timing input, not a parity one)."""
    proj_inv = np.array(fi.projInv[:], np.float64).reshape(4, 4).T
    view_inv = np.array(fi.viewInv[:], np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:height, 0:width]
    clip = np.stack([(xs.reshape(-1) + 0.5) / width * 2 - 1, (ys.reshape(-1) + 0.5) / height * 2 - 1, -np.ones(width * height), np.ones(width * height)], 1)
    view = clip @ proj_inv.T
    view /= view[:, 3:4]
    origin = view_inv[:3, 3]
    d = (view @ view_inv.T)[:, :3] - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(width * height, qu.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["tMin"], rays["tMax"] = origin, d, 0.0, np.inf
    return rays


LAUNCHES = 20  # per timed window: one launch is a fraction of a millisecond, which measures the enqueue as much as the kernel


def best_of(tr, rays_dev, mode, runs=5, **options):
    """ms per launch: the best of `runs` windows of LAUNCHES back-to-back launches between two events, after a warm-up launch.  options:
    alpha / cull / max_hits of PathTracer.query_rays (the _ex entry point); the hit share is that of each ray's first record."""
    stride = options.get("max_hits", 1) if mode == "nearest_k" else 1
    tr.query_rays(rays_dev, mode=mode, **options)
    torch.cuda.synchronize()
    best, hits = None, None
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            hits = tr.query_rays(rays_dev, mode=mode, **options)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b) / LAUNCHES
        best = ms if best is None else min(best, ms)
    hit_share = float((hits[::stride, 12] & 1).float().mean().item())  # (byte 12: the low byte of MiPtRayHit::flags)
    return best, hit_share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detail", type=float, default=0.8, help="bench.py's atrium detail")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--rays", type=int, default=1920 * 1080, help="incoherent rays")
    ap.add_argument("--bvh", type=int, default=0)
    ap.add_argument("--sliver", action="store_true")
    ap.add_argument("--frames", type=int, default=8, help="frames of the k_trace_closest figure")
    ap.add_argument("--alpha", choices=("opaque", "cutoff", "stochastic"), default="opaque", help="alpha mode of the extra rows (mi_pt_query_rays_device_ex)")
    ap.add_argument("--cull", choices=("none", "material"), default="none", help="cull mode of the extra rows")
    ap.add_argument("--max-hits", type=int, default=1, help="> 1: the extra rows are NEAREST_K with this many records per ray")
    a = ap.parse_args()
    w, h = a.size
    with tempfile.TemporaryDirectory() as tmp:
        glb = scenegen.scene_atrium_class(os.path.join(tmp, "atrium.glb"), seed=4321, detail=a.detail, tex_size=64, sliver=a.sliver)  # (bench.py's geometry; texels play no part)
        st = pu.Setup(glb, w, h, max_depth=12)
        tris = qu.SceneTris(st.scene)
        out = {"scene": "atrium_class detail %g%s" % (a.detail, " sliver" if a.sliver else ""), "triangles": len(tris), "bvh": a.bvh, "size": [w, h]}
        tr = ptmod.PathTracer(st.scene, bvh=a.bvh)
        tr.resize(w, h)
        tr.set_frame_info(st.frame_info)
        tr.set_sky(st.sky)
        out["bvh_triangle_slots"] = tr.stats()["bvhTriangleCount"]
        sets = {"coherent": camera_rays(st.frame_info, w, h), "incoherent": qu.make_rays(tris, n=a.rays, seed=7)}
        for name, rays in sets.items():
            dev = torch.from_numpy(qu.as_rows(rays).copy()).cuda()
            for mode in ("closest", "any"):
                ms, share = best_of(tr, dev, mode)
                out["%s_%s" % (name, mode)] = {"rays": len(rays), "ms": round(ms, 4), "Mrays_s": round(len(rays) / ms * 1e-3, 1), "hit_share": round(share, 4)}
            if a.alpha != "opaque" or a.cull != "none" or a.max_hits > 1:
                # the same rays under the options: closest hit, or the max_hits nearest
                mode = "nearest_k" if a.max_hits > 1 else "closest"
                ms, share = best_of(tr, dev, mode, alpha=a.alpha, cull=a.cull, max_hits=a.max_hits)
                out["%s_%s_%s_%s_k%d" % (name, mode, a.alpha, a.cull, a.max_hits)] = {"rays": len(rays), "ms": round(ms, 4), "Mrays_s": round(len(rays) / ms * 1e-3, 1),
                                                                                     "hit_share": round(share, 4)}
        # mi_pt_pick, host form, wall clock: best of five
        ys, xs = np.mgrid[0:h, 0:w]
        xy = np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], 1).astype(np.float32)
        tr.pick(xy)
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            picked = tr.pick(xy)
            wall.append(time.perf_counter() - t0)
        out["pick_host_form"] = {"rays": len(xy), "ms": round(min(wall) * 1e3, 3), "Mrays_s": round(len(xy) / min(wall) * 1e-6, 1),
                                 "hit_share": round(float((picked["renderNode"] >= 0).mean()), 4)}
        # for scale: k_trace_closest's segments per second on the same scene
        tr.enable_timing(True)
        total = 0
        for f in range(a.frames):
            p = st.frame_params(f, total)
            tr.render_frame(p)
            total += p.numSamples
        ft = tr.frame_timing()
        tr.close()
        counted = ptmod.PathTracer(st.scene, bvh=a.bvh, collect_counters=True)
        counted.resize(w, h)
        counted.set_frame_info(st.frame_info)
        counted.set_sky(st.sky)
        total = 0
        for f in range(a.frames):
            p = st.frame_params(f, total)
            counted.render_frame(p)
            total += p.numSamples
        segments = counted.stats()["segments"]
        counted.close()
        out["k_trace_closest"] = {"frames": a.frames, "segments": int(segments), "ms": round(ft["traceClosestMs"], 3),
                                  "Msegments_s": round(segments / max(ft["traceClosestMs"], 1e-9) * 1e-3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
