"""Child process of tests/test_gpu_query_ex.py::test_device_form_with_torch_tensors: the device form of the _ex ray queries
(mi_pt_query_rays_device_ex) fed with torch tensors.  torch is imported BEFORE libmi_pt.so is loaded, so that both use the one HIP runtime torch
brings.
usage: python tests/query_ex_device_child.py <scratch directory>"""
import ctypes as C
import os
import sys

import torch  # (first: see above)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import query_ex_util as qx  # noqa: E402
import query_util as qu  # noqa: E402
from vk_gltf_renderer_amd import _capi as capi  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402


def records(t, k=1):
    r = t.cpu().numpy().view(ptmod.HIT_DTYPE).reshape(-1)
    return r if k == 1 else r.reshape(-1, k)


def main(tmp):
    assert torch.cuda.is_available()
    scene = ptmod.Scene(qx.make_scene("mixed_alpha_glass", tmp))
    st = qu.SceneTris(scene)
    rays = qx.make_rays_ex(st, qx.SceneAlpha(scene, st))
    rows = qu.as_rows(rays)
    for bvh in (0, 1):
        tr = ptmod.PathTracer(scene, bvh=bvh)
        dev = torch.from_numpy(rows.copy()).cuda()
        m0 = tr.memory()
        # default options through the device _ex call: the plain device call's bytes
        o = capi.MiPtQueryOptions()
        tr._l.mi_pt_default_query_options(C.byref(o))
        out = torch.empty((len(rows), 64), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        assert tr._l.mi_pt_query_rays_device_ex(tr._p, C.c_void_p(dev.data_ptr()), len(rows), C.byref(o), C.c_void_p(out.data_ptr()), C.c_void_p(stream or 0)) == 0
        plain = tr.query_rays(dev)
        torch.cuda.synchronize()
        assert records(out).tobytes() == records(plain).tobytes(), bvh
        for kw, k in ((dict(alpha="cutoff"), 1), (dict(alpha="stochastic", seed=9, cull="material"), 1), (dict(mode="any", alpha="cutoff"), 1),
                      (dict(mode="nearest_k", max_hits=3, alpha="cutoff", cull="material"), 3), (dict(mode="nearest_k", max_hits=8), 8)):
            hits = tr.query_rays(dev, **kw)
            assert hits.is_cuda and tuple(hits.shape) == (len(rays) * k, 64) and hits.dtype == torch.uint8, (kw, tuple(hits.shape))
            got = records(hits, k)
            if kw.get("mode") != "any":
                assert got.tobytes() == tr.query_rays(rows, **kw).tobytes(), (bvh, kw)  # the host form's records
                for n in (1, 65, 257):  # a partial last wave and block
                    assert records(tr.query_rays(dev[:n].contiguous(), **kw), k).tobytes() == got[:n].tobytes(), (kw, n)
            else:
                want = tr.query_rays(rows, alpha="cutoff")
                assert (((got["flags"] & 1) != 0) == ((want["flags"] & 1) != 0)).all()
            assert tuple(tr.query_rays(dev[:0], **kw).shape) == (0, 64)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            on_side = tr.query_rays(dev, mode="nearest_k", max_hits=4, alpha="cutoff")
        side.synchronize()
        assert records(on_side, 4).tobytes() == tr.query_rays(rows, mode="nearest_k", max_hits=4, alpha="cutoff").tobytes()
        m1 = tr.memory()
        # the device form allocates nothing: what grew is the host forms' staging of the comparisons above
        assert m1["sceneBytes"] == m0["sceneBytes"] and m1["pathStateBytes"] == m0["pathStateBytes"]
        assert m1["rendererBytes"] - m0["rendererBytes"] == len(rows) * (32 + 8 * 64), (m0, m1)
        tr.close()
    scene.close()
    print("QUERY_EX_DEVICE_OK")


if __name__ == "__main__":
    main(sys.argv[1])
