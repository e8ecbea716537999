"""Cost of bringing new texture images into a resident scene (LABNOTES.md, "Texture image updates"): wall time, the device idle before and
after, of an update of ALL textures of a scene with their mip chains, in four ways:
  host      mi_pt_update_textures from numpy uint8 arrays with MI_PT_TEXTURE_GENERATE_MIPS (staging copy + ingest + mips + footprints),
  device    mi_pt_update_textures_device from torch uint8 tensors already on the GPU (ingest + mips + footprints),
  device32  the same from float32 tensors (quantised by the ingest),
  recreate  what there was before: the host loader's chain (mi_build_mip_chain) + mi_pt_destroy + mi_pt_create.
Two scenes: one quad with one 2048 x 2048 sRGB texture, and scenegen.scene_helmet_class with its 1024 x 1024 textures.  Prints one JSON line per
scene; --out writes a small table.  The mip kernel's own time: MI_PT_BUILD_TIMING=1 prints the update without the flush, and
`rocprofv3 --kernel-trace --stats -- python tools/texture_update_bench.py` gives pt::k_texture_mips per launch.

usage: python tools/texture_update_bench.py [--iters 7] [--size 2048] [--out FILE]"""
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

import parity_util as pu  # noqa: E402
import texture_update_util as tu  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402


def med(v):
    return round(1e3 * sorted(v)[len(v) // 2], 3)


def one_texture_scene(path, size):
    b = scenegen.GlbBuilder()
    y, x = np.mgrid[0:size, 0:size]
    img = np.stack([x % 256, y % 256, (x + y) % 256, np.full_like(x, 255)], -1).astype(np.uint8)  # (compresses well: the file stays small)
    m = b.material({"pbrMetallicRoughness": {"baseColorTexture": {"index": b.texture(b.image(img), b.sampler())}}})
    pos, nrm, uv, idx = scenegen.grid(1, 1, (2.0, 2.0), "z")
    b.node(mesh=b.mesh([b.primitive(pos, idx, nrm, uv, material=m)]))
    b.camera_node((0, 0, 3.0), (0, 0, 0))
    return b.save(path)


def run(name, glb, iters):
    st = pu.Setup(glb, 256, 256, max_depth=2)
    d = st.scene.desc.contents
    tex = [(i, int(d.textures[i].width), int(d.textures[i].height), bool(d.textures[i].srgb), int(d.textures[i].numLevels)) for i in range(int(d.numTextures))]
    result = {"scene": name, "textures": len(tex), "triangles": int(st.scene.num_triangles), "iters": iters, "torch": torch is not None and torch.cuda.is_available(),
              "level0_texels": int(sum(w * h for _, w, h, _, _ in tex))}

    def tracer(scene):
        tr = ptmod.PathTracer(scene)
        tr.resize(256, 256)
        tr.set_frame_info(st.frame_info)
        tr.set_sky(st.sky)
        return tr

    def images(k, dtype=np.uint8):
        r = np.random.default_rng(k)
        if dtype == np.uint8:
            return {i: r.integers(0, 256, (h, w, 4), dtype=np.uint8) for i, w, h, _, _ in tex}
        return {i: r.random((h, w, 4), dtype=np.float32) for i, w, h, _, _ in tex}
    tr = tracer(st.scene)
    timings = {"host": [], "device": [], "device32": []}
    for k in range(iters + 1):  # (the first one warms up, allocates the staging buffer and makes the tables)
        new = images(k)
        tr.synchronize()
        t0 = time.perf_counter()
        tr.update_textures(new)
        tr.synchronize()
        if k:
            timings["host"].append(time.perf_counter() - t0)
    result["launches_per_call"] = tr.texture_update_info()["launches"]
    if result["torch"]:
        for key, dtype in (("device", np.uint8), ("device32", np.float32)):
            for k in range(iters + 1):
                new = {i: torch.from_numpy(a).cuda() for i, a in images(100 + k, dtype).items()}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.update_textures(new)
                tr.synchronize()
                if k:
                    timings[key].append(time.perf_counter() - t0)
    info = tr.texture_update_info()
    result["texels_per_call"] = info["texelsWritten"] // info["calls"]
    tr.close()
    recreate, chain_only = [], []
    for k in range(iters + 1):
        new = images(200 + k)
        t0 = time.perf_counter()
        chains = {i: tu.host_chain(new[i], srgb) for i, _, _, srgb, _ in tex}
        t1 = time.perf_counter()
        holder, keep = tu.textured_desc(st.scene, chains)
        fresh = tracer(holder)  # (destroy is the close() below, timed with it)
        fresh.synchronize()
        fresh.close()
        if k:
            recreate.append(time.perf_counter() - t0)
            chain_only.append(t1 - t0)
        del keep
    for key, v in timings.items():
        if v:
            result[key + "_ms"] = med(v)
    result["recreate_ms"], result["recreate_host_chain_ms"] = med(recreate), med(chain_only)
    # the mip kernel reads every generated level's source once and writes the level: 4 B per source texel + 4 B per written texel
    generated = result["texels_per_call"] - result["level0_texels"]
    result["mip_bytes"] = 4 * (result["texels_per_call"] - len(tex)) + 4 * generated  # (the last level, one texel, is no source)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        rows.append(run("one %d x %d sRGB texture" % (a.size, a.size), one_texture_scene(os.path.join(tmp, "one.glb"), a.size), a.iters))
        print(json.dumps(rows[-1]), flush=True)
        rows.append(run("helmet class", scenegen.scene_helmet_class(os.path.join(tmp, "helmet.glb")), a.iters))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("texture image update of all textures of a scene with generated mip chains, one MI355X, wall time, median of %d\n" % a.iters)
            for r in rows:
                f.write("\n%s: %d textures, %.2f M texels in level 0, %.2f M written per call, %d launches per call, %d triangles\n" % (
                    r["scene"], r["textures"], r["level0_texels"] / 1e6, r["texels_per_call"] / 1e6, r["launches_per_call"], r["triangles"]))
                f.write("%-52s %9.3f ms\n" % ("mi_pt_update_textures (host uint8)", r["host_ms"]))
                if r["torch"]:
                    f.write("%-52s %9.3f ms\n" % ("mi_pt_update_textures_device (uint8 tensor)", r["device_ms"]))
                    f.write("%-52s %9.3f ms\n" % ("mi_pt_update_textures_device (float32 tensor)", r["device32_ms"]))
                f.write("%-52s %9.3f ms  (host chain alone %.3f ms)\n" % ("mi_build_mip_chain + mi_pt_destroy + mi_pt_create", r["recreate_ms"], r["recreate_host_chain_ms"]))


if __name__ == "__main__":
    main()
