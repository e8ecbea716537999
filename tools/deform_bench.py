"""Cost of an animated frame with skins and morph targets (LABNOTES.md, "Skinning and morph targets on the device"): on
scenegen.scene_skinned_large, wall time of the deformation alone (mi_pt_update_deformation with the deferred build), of the rebuild alone
(mi_pt_update_render_nodes), and of a whole animated frame (deform + rebuild + one rendered frame) against a node-transform-only frame of
the same scene (rebuild + one rendered frame), with the bytes the deformation kernel must move at each pose.  Prints one JSON line.  Kernel
time: run under `rocprofv3 --kernel-trace --stats -- python tools/deform_bench.py` and read pt::k_deform.

usage: python tools/deform_bench.py [--tess 240] [--frames 10] [--size 1920 1080]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import parity_util as pu  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402


def kernel_bytes(d):
    """Bytes k_deform reads and writes for the current frame tables (csrc/device/deform.hip): per vertex the base record (16 B, +16 with
    normals, +16 with tangents), influences (8 + 16 B), 12 B per delta stream of every target with a non-zero weight; written: the position
    stream (12) and float4 0 of the interleaved record (16), normals 12 + 8, tangents 16 + 16."""
    w = np.ctypeslib.as_array(d.morphWeights, (d.numMorphWeights,)) if d.numMorphWeights else np.zeros(0)
    total = 0
    for i in range(d.numPrims):
        p = d.prims[i]
        n, t = bool(p.baseNormals), bool(p.baseTangents)
        active = int(np.count_nonzero(w[p.morphWeightOffset:p.morphWeightOffset + p.numTargets])) if p.numTargets else 0
        streams = 1 + bool(p.normalDeltas) + bool(p.tangentDeltas)
        per = 16 + 16 * n + 16 * t + (24 if p.joints else 0) + 12 * streams * active + 28 + 20 * n + 32 * t
        total += per * p.vertexCount
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tess", type=int, default=240)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--accel-update", choices=("rebuild", "refit", "auto"), default="rebuild",
                    help="mi_pt_set_accel_update mode: with refit / auto, rebuild_ms is the time of the acceleration update (a refit)")
    ap.add_argument("--ratio", type=float, default=1.5, help="AUTO's rebuild cost ratio")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        glb = scenegen.scene_skinned(os.path.join(tmp, "skinned_large.glb"), tess=a.tess)
        st = pu.Setup(glb, a.size[0], a.size[1], max_depth=5)
        d = st.scene.deformation
        verts = sum(d.prims[i].vertexCount for i in range(d.numPrims))
        tr = ptmod.PathTracer(st.scene)
        tr.resize(*a.size)
        tr.set_frame_info(st.frame_info)
        tr.set_sky(st.sky)
        tr.set_deformation(st.scene)
        tr.set_accel_update(a.accel_update, a.ratio)
        desc = st.scene.desc.contents
        sah = []
        t_def, t_rebuild, t_anim, t_nodes, moved = [], [], [], [], []
        times = [0.1 + 2.8 * f / max(a.frames - 1, 1) for f in range(a.frames)]
        for f, t in enumerate([0.05] + times):  # (the first one warms up)
            st.scene.update_animation(0, t)
            tr.synchronize()
            t0 = time.perf_counter()
            tr.update_deformation(d.jointMatrices, d.morphWeights, defer_build=True)
            t1 = time.perf_counter()
            tr.update_render_nodes(desc.renderNodes, desc.numRenderNodes, desc.renderNodeVisible)
            tr.update_lights(desc.lights, desc.numLights)
            t2 = time.perf_counter()
            info = tr.accel_info()
            if f and info["sahCostAtBuild"] > 0:
                sah.append(round(info["sahCost"] / info["sahCostAtBuild"], 4))
            tr.render_frame(st.frame_params(0, 0))
            tr.synchronize()
            t3 = time.perf_counter()
            # the node-transform-only frame of the same pose: rebuild + render
            tr.update_render_nodes(desc.renderNodes, desc.numRenderNodes, desc.renderNodeVisible)
            tr.update_lights(desc.lights, desc.numLights)
            tr.render_frame(st.frame_params(0, 0))
            tr.synchronize()
            t4 = time.perf_counter()
            if f:
                t_def.append(t1 - t0)
                t_rebuild.append(t2 - t1)
                t_anim.append(t3 - t0)
                t_nodes.append(t4 - t3)
                moved.append(kernel_bytes(d))
        tr.close()

    def med(v):
        return round(1e3 * sorted(v)[len(v) // 2], 3)
    print(json.dumps({"deformed_vertices": verts, "triangles": st.scene.num_triangles, "size": list(a.size), "frames": a.frames,
                      "kernel_bytes_min": min(moved), "kernel_bytes_max": max(moved), "deform_call_ms": med(t_def), "rebuild_ms": med(t_rebuild),
                      "animated_frame_ms": med(t_anim), "node_only_frame_ms": med(t_nodes), "accel_update": a.accel_update,
                      "accel_info": info, "sah_ratio_per_pose": sah}))


if __name__ == "__main__":
    main()
