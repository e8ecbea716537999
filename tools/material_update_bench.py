"""Cost of a material update (LABNOTES.md, "Material updates"): on the street-class and atrium-class stand-ins of bench.py, wall time of
mi_pt_update_materials followed by a synchronisation for (i) a factor-only update (no kernel) and (ii) an update that patches every triangle
slot (one material set on every render node, its instance flags and alpha state changed), against what the same change cost before the call
existed: destroying the instance and mi_pt_create again -- and the build part of that alone, from the MI_PT_BUILD_TIMING lines when the
variable is set.  Prints one JSON line per scene.  Kernel time: run (ii) alone under
`rocprofv3 --kernel-trace --stats -- python tools/material_update_bench.py --scene street --only patch` and read pt::k_patch_materials;
the bytes it moves stand in the output (slots x (48 read + 52 written)).

usage: python tools/material_update_bench.py [--scene street atrium] [--repeat 5] [--only factor|patch|create]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from vk_gltf_renderer_amd import _capi as capi  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402

SCENES = {"street": ("scene_street_class", dict(seed=777, detail=1.27, tex_size=256)),   # bench.py: WORKLOADS["street"]
          "atrium": ("scene_atrium_class", dict(seed=4321, detail=0.8, tex_size=512))}   # ... ["atrium"]


def tables(scene):
    d = scene.desc.contents
    mats = (capi.MiGltfShadeMaterial * d.numMaterials)()
    C.memmove(mats, d.materials, C.sizeof(mats))
    infos = (capi.MiGltfTextureInfo * d.numTextureInfos)()
    C.memmove(infos, d.textureInfos, C.sizeof(infos))
    return mats, infos


def med(v):
    return round(1e3 * sorted(v)[len(v) // 2], 3) if v else None


def run(name, a):
    gen, kw = SCENES[name]
    with tempfile.TemporaryDirectory() as tmp:
        scene = ptmod.Scene(getattr(scenegen, gen)(os.path.join(tmp, name + ".glb"), **kw))
    d = scene.desc.contents
    # one material on every render node, so that (ii) dirties every slot: the most used OPAQUE one
    use = {}
    for n in range(d.numRenderNodes):
        use[d.renderNodes[n].materialID] = use.get(d.renderNodes[n].materialID, 0) + 1
    wide = max((m for m in use if d.materials[max(m, 0)].alphaMode == 0), key=lambda m: use[m])
    for n in range(d.numRenderNodes):
        d.renderNodes[n].materialID = wide
    t0 = time.perf_counter()
    tr = ptmod.PathTracer(scene)
    tr.synchronize()
    create_first = time.perf_counter() - t0
    slots = tr.stats()["bvhTriangleCount"]
    mats, infos = tables(scene)
    out = {"scene": name, "triangles": scene.num_triangles, "triangle_slots": slots, "render_nodes": d.numRenderNodes, "materials": d.numMaterials,
           "patch_kernel_bytes": slots * (48 + 52), "create_first_ms": round(1e3 * create_first, 3)}
    t_factor, t_patch, t_create = [], [], []
    for k in range(a.repeat + 1):  # (the first round warms up)
        if a.only in (None, "factor"):
            mats[wide].pbrRoughnessFactor = 0.2 + 0.05 * k
            mats[wide].emissiveFactor[0] = 0.01 * k
            t0 = time.perf_counter()
            tr.update_materials(mats, len(mats), infos, len(infos))
            tr.synchronize()
            t_factor.append(time.perf_counter() - t0)
        if a.only in (None, "patch"):
            # BLEND <-> MASK with another cutoff, single <-> double sided: the alpha records stay allocated, flags and records of every slot change
            mats[wide].alphaMode = 2 if k % 2 == 0 else 1
            mats[wide].alphaCutoff = 0.3 + 0.01 * k
            mats[wide].doubleSided = k % 2
            mats[wide].pbrBaseColorFactor[3] = 0.9
            t0 = time.perf_counter()
            tr.update_materials(mats, len(mats), infos, len(infos))
            tr.synchronize()
            t_patch.append(time.perf_counter() - t0)
            out["builds_after_patches"] = tr.accel_info()["builds"]
        if a.only in (None, "create"):
            # the same change without the call: destroy + create on the new tables
            C.memmove(d.materials, mats, C.sizeof(mats))
            t0 = time.perf_counter()
            tr.close()
            tr = ptmod.PathTracer(scene)
            tr.synchronize()
            t_create.append(time.perf_counter() - t0)
    tr.close()
    out.update(factor_only_ms=med(t_factor[1:]), patch_all_slots_ms=med(t_patch[1:]), destroy_create_ms=med(t_create[1:]))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", nargs="+", default=["street", "atrium"], choices=sorted(SCENES))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--only", choices=("factor", "patch", "create"), default=None)
    a = ap.parse_args()
    for name in a.scene:
        run(name, a)


if __name__ == "__main__":
    main()
