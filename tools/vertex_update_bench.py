"""Cost of bringing new vertices into a resident scene (LABNOTES.md, "Caller-driven vertices"): on scenegen.scene_skinned_large-sized geometry
(no deformation tables: every primitive is declared with mi_pt_set_vertex_updates), wall time of an update of ALL primitives -- positions,
and the normals and tangents of the primitives that have them -- in three ways:
  host      mi_pt_update_vertices from numpy arrays (staging copy + ingest launch + acceleration update),
  device    mi_pt_update_vertices_device from torch tensors already on the GPU (ingest launch + acceleration update),
  recreate  mi_pt_destroy + mi_pt_create of the same vertices (every texture and stream uploaded again, a full build),
each under MI_PT_ACCEL_REBUILD and MI_PT_ACCEL_REFIT (recreate always builds).  Prints one JSON line; --out writes a small table.
Kernel time: run under `rocprofv3 --kernel-trace --stats -- python tools/vertex_update_bench.py` and read pt::k_vertex_ingest.

usage: python tools/vertex_update_bench.py [--tess 240] [--iters 7] [--size 1920 1080] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

try:
    import torch  # (before libmi_pt.so is loaded: both then use the one HIP runtime torch brings)
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import deform_util as du  # noqa: E402
import parity_util as pu  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402


def med(v):
    return round(1e3 * sorted(v)[len(v) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tess", type=int, default=240)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {"size": list(a.size), "iters": a.iters, "torch": torch is not None and torch.cuda.is_available()}
    with tempfile.TemporaryDirectory() as tmp:
        glb = scenegen.scene_skinned(os.path.join(tmp, "skinned_large.glb"), tess=a.tess)
        st = pu.Setup(glb, a.size[0], a.size[1], max_depth=5)
        d = st.scene.desc.contents
        prims = [i for i in range(int(d.numRenderPrimitives)) if d.renderPrimitives[i].vertexCount and d.renderPrimitives[i].positions]

        def tracer(scene):
            tr = ptmod.PathTracer(scene)
            tr.resize(*a.size)
            tr.set_frame_info(st.frame_info)
            tr.set_sky(st.sky)
            return tr
        tr = tracer(st.scene)
        rest = {p: tr.read_vertices(p) for p in prims}
        result["vertices"] = int(sum(len(rest[p][0]) for p in prims))
        result["triangles"] = int(st.scene.num_triangles)
        result["bytes_per_update"] = int(sum(sum(s.nbytes for s in rest[p] if s is not None) for p in prims))

        def pose(k):  # a breathing scale about the origin: every vertex moves, the topology of the tree stays sensible
            s = np.float32(1.0 + 0.01 * np.sin(0.7 * k))
            return {p: ((rest[p][0] * s).astype(np.float32), rest[p][1], rest[p][2]) for p in prims}
        tr.set_vertex_updates(prims)
        for mode in ("rebuild", "refit"):
            tr.set_accel_update(mode)
            host, dev = [], []
            for k in range(a.iters + 1):  # (the first one warms up, and allocates the staging buffer)
                streams = pose(k)
                tr.synchronize()
                t0 = time.perf_counter()
                tr.update_vertices(streams)
                tr.synchronize()
                if k:
                    host.append(time.perf_counter() - t0)
            result["host_%s_ms" % mode] = med(host)
            if result["torch"]:
                for k in range(a.iters + 1):
                    streams = {p: tuple(None if s is None else torch.from_numpy(s).cuda() for s in v) for p, v in pose(k + 100).items()}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr.update_vertices(streams)
                    tr.synchronize()
                    if k:
                        dev.append(time.perf_counter() - t0)
                result["device_%s_ms" % mode] = med(dev)
            result["accel_%s" % mode] = {k: v for k, v in tr.accel_info().items() if k in ("builds", "refits", "trianglesMoved")}
        result["update_info"] = tr.vertex_update_info()
        tr.close()
        recreate = []
        for k in range(a.iters + 1):
            holder, keep = du.posed_desc(st.scene, pose(k + 200))
            t0 = time.perf_counter()
            fresh = tracer(holder)  # (destroy is the close() below, timed with it)
            fresh.synchronize()
            fresh.close()
            if k:
                recreate.append(time.perf_counter() - t0)
            del keep
        result["recreate_ms"] = med(recreate)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("vertex update of all primitives, one MI355X: %d vertices, %d triangles, %.1f MB of streams per update, %dx%d, median of %d\n" % (
                result["vertices"], result["triangles"], result["bytes_per_update"] / 1e6, a.size[0], a.size[1], a.iters))
            f.write("%-28s %12s %12s\n" % ("", "REBUILD", "REFIT"))
            f.write("%-28s %9.3f ms %9.3f ms\n" % ("mi_pt_update_vertices", result["host_rebuild_ms"], result["host_refit_ms"]))
            if result["torch"]:
                f.write("%-28s %9.3f ms %9.3f ms\n" % ("mi_pt_update_vertices_device", result["device_rebuild_ms"], result["device_refit_ms"]))
            f.write("%-28s %9.3f ms %12s\n" % ("mi_pt_destroy + mi_pt_create", result["recreate_ms"], "(a build)"))


if __name__ == "__main__":
    main()
