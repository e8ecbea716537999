"""Child process of tests/test_gpu_env_update.py::test_device_form_with_torch_tensors: the device form of the environment updates
(mi_pt_update_environment_device) fed with torch tensors.  torch is imported BEFORE libmi_pt.so is loaded, so that both use the one HIP
runtime torch brings.
usage: python tests/env_update_device_child.py <scratch directory>"""
import ctypes as C
import os
import sys

import torch  # (first: see above)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import env_update_util as eu  # noqa: E402
import parity_util as pu  # noqa: E402
from vk_gltf_renderer_amd import _capi as capi  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402

MEMORY_KEYS = ("sceneBytes", "rendererBytes", "pathStateBytes")


def same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def offset_tensor(a, skip):
    """The array as a contiguous device tensor that starts `skip` floats into its allocation."""
    buf = torch.empty(a.size + skip, dtype=torch.float32, device="cuda")
    buf[skip:] = torch.from_numpy(a.reshape(-1).copy()).cuda()
    t = buf[skip:].view(a.shape)
    assert t.is_contiguous()
    return t


def main(tmp):
    assert torch.cuda.is_available()
    st = pu.Setup(os.path.join(ROOT, "assets", "Box.glb"), 16, 16, max_depth=2)
    host, dev = ptmod.PathTracer(st.scene), ptmod.PathTracer(st.scene)
    cases = eu.SMALL_CASES + ((1500, 750, "std_env"),)
    for case in cases:
        px = eu.load_hdr_pixels() if case[2] == "std_env" else eu.make_pixels(*case)
        px4 = np.concatenate([px, np.full(px.shape[:2] + (1,), np.nan, np.float32)], -1)
        host.update_environment(px)
        want = host.read_environment()
        t3, t4, t3_off = torch.from_numpy(px).cuda(), torch.from_numpy(px4).cuda(), offset_tensor(px, 1)
        assert t3_off.data_ptr() % 16 != 0 and t3_off.data_ptr() % 4 == 0
        torch.cuda.synchronize()
        dev.update_environment(t3)
        m0 = dev.memory()
        assert same(dev.read_environment(), want), ("rgb tensor", case)
        for name, t in (("rgba tensor", t4), ("rgb tensor again", t3), ("rgb tensor off a 16-byte boundary", t3_off)):
            dev.update_environment(t)
            assert same(dev.read_environment(), want), (name, case)
        assert all(dev.memory()[k] == m0[k] for k in MEMORY_KEYS), case  # in place: nothing allocated
        assert dev.environment_update_info()["texelsSanitised"] == 0

    # ---- what the device form cannot validate, it sanitises; the host form refuses the same data
    px = eu.make_pixels(65, 33, "tail")
    bad = px.copy()
    bad[0, 0, 1], bad[5, 7, 0], bad[32, 64, 2], bad[9, 9, :] = np.nan, -1.0, np.inf, (np.nan, -np.inf, -2.0)
    replaced = ~(np.isfinite(bad) & (bad >= 0))
    clean = bad.copy()
    clean[replaced] = 0.0
    for t in (torch.from_numpy(bad).cuda(), torch.from_numpy(np.concatenate([bad, np.zeros((33, 65, 1), np.float32)], -1)).cuda()):
        torch.cuda.synchronize()
        dev.update_environment(t)
        got = dev.read_environment()
        info = dev.environment_update_info()
        assert info["texelsSanitised"] == 4, info
        assert (got[0][..., :3][replaced] == 0).all() and np.isfinite(got[0]).all() and np.isfinite(got[3])
        eu.check_table(clean, *got)
        eu.check_against_host_route(clean, got[0], got[3])
    host.update_environment(clean)
    assert same(host.read_environment(), got)
    before = ([np.asarray(x).tobytes() for x in host.read_environment()], host.environment_update_info())
    try:
        host.update_environment(bad)
        raise SystemExit("the host form accepted a NaN")
    except ptmod.MiError as e:
        assert "rc=-1" in str(e) and "not finite" in str(e), str(e)
    assert ([np.asarray(x).tobytes() for x in host.read_environment()], host.environment_update_info()) == before

    # ---- the binding refuses what is no float32 tensor on the device; the library a misaligned pointer, with nothing changed
    t = torch.from_numpy(px).cuda()
    for wrong in (t.double(), t[:, ::2], t.cpu(), t[..., :2].contiguous()):
        try:
            dev.update_environment(wrong)
            raise SystemExit("a bad tensor was accepted: %r" % (wrong.shape,))
        except ValueError:
            pass
    before = [np.asarray(x).tobytes() for x in dev.read_environment()]
    t4_off = offset_tensor(np.concatenate([px, np.zeros((33, 65, 1), np.float32)], -1), 1)
    assert t4_off.data_ptr() % 16 != 0
    try:
        dev.update_environment(t4_off)
        raise SystemExit("a misaligned RGBA pointer was accepted")
    except ptmod.MiError as e:
        assert "rc=-1" in str(e) and "aligned" in str(e), str(e)
    u = capi.MiPtEnvironmentUpdate()
    u.width, u.height, u.channels, u.pixels = 65, 33, 3, t.data_ptr() + 2
    assert dev._l.mi_pt_update_environment_device(dev._p, C.byref(u)) == -1
    assert [np.asarray(x).tobytes() for x in dev.read_environment()] == before
    host.close()
    dev.close()
    print("ENV_UPDATE_DEVICE_OK")


if __name__ == "__main__":
    main(sys.argv[1])
