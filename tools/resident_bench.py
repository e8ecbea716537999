"""Cost of visibility and material-id updates with resident mode on and off (LABNOTES.md, "Resident mode"): on the street-class and
atrium-class stand-ins of bench.py, under REFIT, median wall time of mi_pt_update_render_nodes followed by a synchronisation for
  1. an update that hides the largest instance,
  2. an update that shows it again,
  3. an update that gives every render node another material id (the next material of the table with the same transmissive bit, so that no
     update falls back to a build for a reason of its own),
each with mi_pt_set_accel_resident on (a refit / a patch) and off (the rebuild every such update costs without it: the baseline); and
  4. the frame rate with that instance hidden inside the resident tree against a fresh instance whose tree was built without it: the price of
     carrying hidden geometry.
Prints one JSON line per scene.

usage: python tools/resident_bench.py [--scene street atrium] [--repeat 5] [--size 1920 1080] [--frames 8]"""
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

SCENES = {"street": ("scene_street_class", dict(seed=777, detail=1.27, tex_size=256)),   # bench.py: WORKLOADS["street"]
          "atrium": ("scene_atrium_class", dict(seed=4321, detail=0.8, tex_size=512))}   # ... ["atrium"]


def med(v):
    return round(1e3 * sorted(v)[len(v) // 2], 3) if v else None


def tracer(st, size):
    tr = ptmod.PathTracer(st.scene)
    tr.resize(*size)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    return tr


def timed_update(tr, d):
    tr.synchronize()
    t0 = time.perf_counter()
    tr.update_render_nodes(d.renderNodes, d.numRenderNodes, d.renderNodeVisible)
    tr.synchronize()
    return time.perf_counter() - t0


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


def run(name, a):
    gen, kw = SCENES[name]
    with tempfile.TemporaryDirectory() as tmp:
        st = pu.Setup(getattr(scenegen, gen)(os.path.join(tmp, name + ".glb"), **kw), a.size[0], a.size[1], max_depth=5)
    d = st.scene.desc.contents
    n = int(d.numRenderNodes)
    counts = [int(d.renderPrimitives[d.renderNodes[i].renderPrimID].triangleCount) if d.renderNodes[i].renderPrimID >= 0 else 0 for i in range(n)]
    big = int(np.argmax(counts))
    # the material every node switches to and back from: the next one of the table with the same transmissive bit
    groups = {}
    for m in range(d.numMaterials):
        groups.setdefault(d.materials[m].transmissionFactor > 0.01, []).append(m)
    nxt = {m: g[(g.index(m) + 1) % len(g)] for g in groups.values() for m in g}
    home = [max(0, d.renderNodes[i].materialID) for i in range(n)]
    out = {"scene": name, "triangles": st.scene.num_triangles, "render_nodes": n, "hidden_instance_triangles": counts[big],
           "nodes_switched": sum(1 for m in home if nxt[m] != m)}
    for mode in ("resident", "rebuild"):
        tr = tracer(st, a.size)
        tr.set_accel_update("refit")
        if mode == "resident":
            tr.set_accel_resident(True)
        builds0 = tr.accel_info()["builds"]
        out[mode + "_triangle_slots"] = tr.stats()["bvhTriangleCount"]
        out[mode + "_scene_bytes"] = tr.memory()["sceneBytes"]
        t_hide, t_show, t_mat = [], [], []
        for k in range(a.repeat + 1):  # (the first round warms up)
            d.renderNodeVisible[big] = 0
            t_hide.append(timed_update(tr, d))
            if k == a.repeat and mode == "resident":
                out["msamples_s_hidden_in_resident_tree"] = round(speed(tr, st, a.size, a.frames), 1)
                fresh = tracer(st, a.size)  # (from the same tables: its tree holds the visible nodes only)
                out["msamples_s_fresh_tree_without_it"] = round(speed(fresh, st, a.size, a.frames), 1)
                out["fresh_triangle_slots"] = fresh.stats()["bvhTriangleCount"]
                fresh.close()
            d.renderNodeVisible[big] = 1
            t_show.append(timed_update(tr, d))
            for i in range(n):
                d.renderNodes[i].materialID = nxt[home[i]] if k % 2 == 0 else home[i]
            t_mat.append(timed_update(tr, d))
        for i in range(n):
            d.renderNodes[i].materialID = home[i]
        info = tr.accel_info()
        out[mode + "_builds_during_updates"] = info["builds"] - builds0
        if mode == "resident":
            out["resident_info"] = tr.accel_resident_info()
        tr.close()
        out[mode + "_hide_ms"], out[mode + "_show_ms"], out[mode + "_material_ids_ms"] = med(t_hide[1:]), med(t_show[1:]), med(t_mat[1:])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", nargs="+", default=["street", "atrium"], choices=sorted(SCENES))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    for name in a.scene:
        run(name, a)


if __name__ == "__main__":
    main()
