"""Child process of tests/test_gpu_query.py::test_device_form_with_torch_tensors: the device form of the ray queries (mi_pt_query_rays_device)
fed with torch tensors.  torch is imported BEFORE libmi_pt.so is loaded, so that both use the one HIP runtime torch brings.
usage: python tests/query_device_child.py <scratch directory>"""
import os
import sys

import torch  # (first: see above)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import parity_util as pu  # noqa: E402
import query_util as qu  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402

W, H = 128, 96
HIT = 1


def records(t):
    return t.cpu().numpy().view(ptmod.HIT_DTYPE).reshape(-1)


def main(tmp):
    assert torch.cuda.is_available()
    # a torch tensor goes in; the records equal the host form's, in both trees
    scene = ptmod.Scene(scenegen.scene_variants(os.path.join(tmp, "variants.glb")))
    st = qu.SceneTris(scene)
    rays = qu.make_rays(st)
    rows = qu.as_rows(rays)
    for bvh in (0, 1):
        tr = ptmod.PathTracer(scene, bvh=bvh)
        m0 = tr.memory()
        dev = torch.from_numpy(rows.copy()).cuda()
        hits = tr.query_rays(dev)
        assert hits.is_cuda and tuple(hits.shape) == (len(rays), 64) and hits.dtype == torch.uint8
        got = records(hits)
        m1 = tr.memory()
        assert all(m1[k] == m0[k] for k in ("sceneBytes", "rendererBytes", "pathStateBytes")), (m0, m1)  # the device form allocates nothing
        whole = tr.query_rays(rows)
        assert got.tobytes() == whole.tobytes(), bvh
        assert (got["renderNode"] >= 0).sum() > 500
        for n in (1, 63, 65, 257):  # a partial last wave and block
            assert records(tr.query_rays(dev[:n].contiguous())).tobytes() == whole[:n].tobytes(), n
        anyhit = records(tr.query_rays(dev, mode="any"))
        assert (((anyhit["flags"] & HIT) != 0) == ((whole["flags"] & HIT) != 0)).all()
        assert tuple(tr.query_rays(dev[:0]).shape) == (0, 64)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # (the binding takes torch's current stream)
            on_side = tr.query_rays(dev)
        side.synchronize()
        assert records(on_side).tobytes() == whole.tobytes()
        try:
            tr.query_rays(torch.zeros((4, 7), dtype=torch.float32, device="cuda"))
            raise SystemExit("a (4, 7) tensor was accepted")
        except ValueError:
            pass
        tr.close()
    scene.close()
    # a query between queued frames leaves the accumulator alone
    glb = scenegen.scene_animated(os.path.join(tmp, "animated.glb"))
    s = pu.Setup(glb, W, H, max_depth=3)
    rays = qu.make_rays(qu.SceneTris(s.scene), n=1000, seed=11)
    dev = torch.from_numpy(qu.as_rows(rays).copy()).cuda()
    xy = np.stack([np.arange(100) + 0.5, np.full(100, 40.5)], 1)
    images, seen = [], []
    for with_query in (False, True):
        tr = ptmod.PathTracer(s.scene)
        tr.resize(W, H)
        tr.set_frame_info(s.frame_info)
        tr.set_sky(s.sky)
        tr.set_frame_queue(4)
        total = 0
        for f in range(6):
            p = s.frame_params(f, total)
            tr.render_frame(p)
            total += p.numSamples
            if with_query and f in (0, 2):  # frame 0, then frames 1 and 2, are pending when these arrive
                seen.append(records(tr.query_rays(dev)))
                seen.append(tr.pick(xy))
        images.append(tr.read_accum())
        if with_query:
            assert seen[0].tobytes() == seen[2].tobytes() == tr.query_rays(qu.as_rows(rays)).tobytes()
            assert seen[1].tobytes() == seen[3].tobytes()
        tr.close()
    assert (images[0] == images[1]).all() and np.isfinite(images[0]).all() and images[0][..., :3].max() > 0
    print("QUERY_DEVICE_OK")


if __name__ == "__main__":
    main(sys.argv[1])
