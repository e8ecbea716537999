"""Times an environment update by its three routes, from the same pixels:
  device   mi_pt_update_environment_device from a torch tensor on the GPU
  host     mi_pt_update_environment from a numpy array (staged, then the same kernels)
  parent   mi_hdr_from_pixels (the sequential alias loop on one CPU thread) + mi_pt_set_environment (upload of the finished tables)
Method: warm-up calls, then the median of --runs calls, the device synchronised before and after each call (the library synchronises inside
the update calls too).  --split runs the device route once more in a child with MI_PT_BUILD_TIMING set, where the library synchronises after
each of the six launches and prints its time: the per-kernel split (medians).  The one pass condition: the device route at 2048 x 1024 is
faster than the parent's.
usage: python tools/time_env_update.py [--sizes 2048x1024,4096x2048] [--runs 15] [--warmup 3] [--split] [--out profiles/env_update_times.txt]"""
import argparse
import os
import re
import subprocess
import sys
import time

import torch  # (before libmi_pt.so: both then use the HIP runtime torch brings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402


def sky_like(width, height, pattern):
    """A tail-heavy map (a sun over a gradient), or the one-hot map whose binary searches all end at one heavy texel."""
    if pattern == "onehot":
        px = np.zeros((height, width, 3), np.float32)
        px[height // 2, width // 3] = 3.0
        return px
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    rng = np.random.default_rng(7)
    px = np.stack([0.2 + 0.5 * y / height, 0.3 + 0.4 * y / height, 0.9 - 0.6 * y / height], -1) * rng.random((height, width, 1), dtype=np.float32) ** 4
    px[height // 5:height // 5 + 8, width // 2:width // 2 + 8] = 6.0e4
    return np.ascontiguousarray(px, np.float32)


def median_ms(call, runs, warmup):
    times = []
    for k in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def split_child(width, height, pattern, runs):
    tr = ptmod.PathTracer(ptmod.Scene(os.path.join(ROOT, "assets", "Box.glb")))
    t = torch.from_numpy(sky_like(width, height, pattern)).cuda()
    torch.cuda.synchronize()
    for _ in range(runs):
        tr.update_environment(t)
    tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x1024,4096x2048")
    ap.add_argument("--patterns", default="sky,onehot")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--split-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.split_child:
        w, h, pattern = a.split_child.split(",")
        split_child(int(w), int(h), pattern, a.runs)
        return 0
    lines, ok = [], True
    scene = ptmod.Scene(os.path.join(ROOT, "assets", "Box.glb"))
    for size in a.sizes.split(","):
        width, height = (int(v) for v in size.split("x"))
        for pattern in a.patterns.split(","):
            px = sky_like(width, height, pattern)
            tr = ptmod.PathTracer(scene)
            t = torch.from_numpy(px).cuda()
            dev = median_ms(lambda: tr.update_environment(t), a.runs, a.warmup)
            info = tr.environment_update_info()
            host = median_ms(lambda: tr.update_environment(px), a.runs, a.warmup)

            def parent():
                hdr = ptmod.HdrEnvironment(pixels=px)
                tr.set_environment(hdr)
                hdr.close()
            par = median_ms(parent, max(3, a.runs // 3), 1)
            tr.close()
            lines.append("%dx%d %-6s  device %8.3f ms (min %.3f max %.3f)  host %8.3f ms (min %.3f max %.3f)  parent route %9.3f ms (min %.3f max %.3f)  "
                         "launches %d light %d heavy %d scratch %.2f B/texel" % ((width, height, pattern) + dev + host + par + (
                             info["launches"], info["lightTexels"], info["heavyTexels"], info["scratchBytes"] / (width * height))))
            print(lines[-1], flush=True)
            if (width, height) == (2048, 1024):
                ok = ok and dev[0] < par[0]
            if a.split:
                env = dict(os.environ, MI_PT_BUILD_TIMING="1")
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--split-child", "%d,%d,%s" % (width, height, pattern), "--runs", str(a.runs)],
                                   env=env, capture_output=True, text=True, timeout=600)
                passes = {}
                for name, ms in re.findall(r"\[mi_pt build\] (env [a-z ]+?)\s+([0-9.]+) ms", r.stderr):
                    passes.setdefault(name, []).append(float(ms))
                lines.append("    per launch, synchronised after each (median ms): " + ", ".join("%s %.3f" % (k, np.median(v)) for k, v in passes.items()))
                print(lines[-1], flush=True)
    lines.append("device route at 2048x1024 faster than the parent's route: %s" % ("yes" if ok else "NO"))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
