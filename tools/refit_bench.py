"""Refit against rebuild (LABNOTES.md, "Refit instead of rebuild"): tree quality and update cost.

1. Tree quality on scenegen.scene_skinned_large: at poses across the clip, an instance in REFIT mode (its tree built at the rest pose, then
   refitted) against a fresh instance created from the posed vertices read back from it.  Per tree: SAH cost over the fresh tree's,
   closest-hit node visits per ray segment and shadow node visits per shadow ray (collectCounters), and Msamples/s at --size, 1 spp, depth 5.
2. Node transforms on scenegen.scene_atrium_class: the largest instance moved every update, median wall time of mi_pt_update_render_nodes in
   REBUILD and in REFIT mode.

Prints one JSON line.  Kernel time of the refit: `rocprofv3 --kernel-trace --stats -- python tools/deform_bench.py --accel-update refit`.

usage: python tools/refit_bench.py [--tess 240] [--size 1920 1080] [--frames 8] [--moves 8]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import deform_util as du  # noqa: E402
import parity_util as pu  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402


def tracer(scene, st, size, counters):
    tr = ptmod.PathTracer(scene, collect_counters=counters)
    tr.resize(*size)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    return tr


def quality(tr, st):
    """(closest-hit node visits per ray segment, shadow node visits per shadow ray) of one 1-spp frame"""
    tr.reset_stats()
    tr.render_frame(st.frame_params(0, 0))
    tr.synchronize()
    s = tr.stats()
    return (s["nodesPrimary"] + s["nodesClosest"]) / max(s["segments"], 1), s["nodesShadow"] / max(s["shadowRays"], 1)


def speed(tr, st, size, frames):
    tr.render_frame(st.frame_params(0, 0))
    tr.synchronize()
    t0 = time.perf_counter()
    total = 0
    for f in range(frames):
        p = st.frame_params(f, total)
        tr.render_frame(p)
        total += p.numSamples
    tr.synchronize()
    return size[0] * size[1] * total / (time.perf_counter() - t0) / 1e6


def skinned_quality(a, tmp):
    glb = scenegen.scene_skinned(os.path.join(tmp, "skinned_large.glb"), tess=a.tess)
    st = pu.Setup(glb, a.size[0], a.size[1], max_depth=5)
    d = st.scene.deformation
    rows = []
    refit = {}
    for counters in (True, False):
        tr = tracer(st.scene, st, a.size, counters)
        tr.set_deformation(st.scene)
        tr.set_accel_update("refit", 1e30)
        refit[counters] = tr
    for t in (0.1, 0.8, 1.5, 2.2, 2.9):
        st.scene.update_animation(0, t)
        for tr in refit.values():
            tr.update_from_scene(st.scene)
        info = refit[True].accel_info()
        streams = {p.renderPrimID: refit[True].read_vertices(p.renderPrimID) for p in du.prims(d)}
        holder, keep = du.posed_desc(st.scene, streams)
        fresh = {}
        for counters in (True, False):
            fresh[counters] = tracer(holder, st, a.size, counters)
            fresh[counters].set_accel_update("auto", 1e30)  # (a build that keeps refit data: its SAH cost, the reference)
        fresh_sah = fresh[True].accel_info()["sahCost"]
        rv, fv = quality(refit[True], st), quality(fresh[True], st)
        rs, fs = speed(refit[False], st, a.size, a.frames), speed(fresh[False], st, a.size, a.frames)
        rows.append({"time": t, "sah_refit_over_build": round(info["sahCost"] / info["sahCostAtBuild"], 4),
                     "sah_refit_over_fresh": round(info["sahCost"] / fresh_sah, 4),
                     "visits_per_segment_refit": round(rv[0], 3), "visits_per_segment_fresh": round(fv[0], 3),
                     "visits_per_shadow_ray_refit": round(rv[1], 3), "visits_per_shadow_ray_fresh": round(fv[1], 3),
                     "msamples_s_refit": round(rs, 1), "msamples_s_fresh": round(fs, 1)})
        for tr in fresh.values():
            tr.close()
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    for tr in refit.values():
        tr.close()
    return {"scene": "scene_skinned_large", "triangles": st.scene.num_triangles, "poses": rows}


def node_moves(a, tmp):
    glb = scenegen.scene_atrium_class(os.path.join(tmp, "atrium.glb"))
    st = pu.Setup(glb, 320, 240, max_depth=2)
    desc = st.scene.desc.contents
    nodes, n = desc.renderNodes, int(desc.numRenderNodes)
    counts = [int(desc.renderPrimitives[nodes[i].renderPrimID].triangleCount) if nodes[i].renderPrimID >= 0 else 0 for i in range(n)]
    big = int(np.argmax(counts))
    M0 = np.array(nodes[big].objectToWorld[:], np.float64).reshape(4, 4).T
    raw = (list(nodes[big].objectToWorld), list(nodes[big].worldToObject))
    out = {"scene": "scene_atrium_class", "triangles": st.scene.num_triangles, "moved_node_triangles": counts[big]}
    for mode in ("rebuild", "refit"):
        tr = tracer(st.scene, st, (320, 240), False)
        tr.set_accel_update(mode)
        times = []
        for k in range(a.moves + 1):
            c, s = np.cos(0.05 * (k + 1)), np.sin(0.05 * (k + 1))
            R = np.eye(4)
            R[0, 0], R[0, 2], R[2, 0], R[2, 2] = c, s, -s, c
            R[:3, 3] = (0.1 * k, 0.0, 0.0)
            M = R @ M0
            nodes[big].objectToWorld[:] = [float(v) for v in M.T.reshape(-1).astype(np.float32)]
            nodes[big].worldToObject[:] = [float(v) for v in np.linalg.inv(M).T.reshape(-1).astype(np.float32)]
            tr.synchronize()
            t0 = time.perf_counter()
            tr.update_render_nodes(nodes, n, desc.renderNodeVisible)
            tr.synchronize()
            if k:
                times.append(time.perf_counter() - t0)
        info = tr.accel_info()
        tr.close()
        nodes[big].objectToWorld[:], nodes[big].worldToObject[:] = raw
        out[mode + "_ms"] = round(1e3 * sorted(times)[len(times) // 2], 3)
        if mode == "refit":
            out["refit_sah_over_build"] = round(info["sahCost"] / info["sahCostAtBuild"], 4)
            out["refits"] = info["refits"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tess", type=int, default=240)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--moves", type=int, default=8)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        res = {"node_moves": node_moves(a, tmp)}
        print(json.dumps(res["node_moves"]), file=sys.stderr, flush=True)
        res["quality"] = skinned_quality(a, tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
