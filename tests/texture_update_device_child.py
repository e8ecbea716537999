"""Child process of tests/test_gpu_texture_update.py::test_device_form_with_torch_tensors: the device form of the texture image updates
(mi_pt_update_textures_device) fed with torch tensors.  torch is imported BEFORE libmi_pt.so is loaded, so that both use the one HIP runtime
torch brings.
usage: python tests/texture_update_device_child.py <scratch directory>"""
import os
import sys

import torch  # (first: see above)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import parity_util as pu  # noqa: E402
import texture_update_util as tu  # noqa: E402
from vk_gltf_renderer_amd import _capi as capi  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd._capi import Visualization as V  # noqa: E402

SIDE = tu.SIDE


def tracer(st):
    tr = ptmod.PathTracer(st.scene)
    tr.resize(SIDE, SIDE)
    tr.set_sky(st.sky)
    return tr


def view(tr, st, rays, name, angle):
    tr.set_camera_rays(rays, unit=True)
    fi = st.frame_info
    fi.visualization = int(V[name])
    tr.set_frame_info(fi)
    p = st.frame_params(0, 0)
    p.pixelAngle = float(angle)
    p.flags = capi.MI_PT_FIRST_FRAME
    tr.render_frame(p)
    return tr.read_accum()


def chain(tr, st, i):
    return [tr.read_texture(i, l) for l in range(int(st.scene.desc.contents.textures[i].numLevels))]


def same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def offset_tensor(a, skip):
    """The array as a contiguous device tensor that starts `skip` elements into its allocation."""
    buf = torch.empty(a.size + skip, dtype=torch.from_numpy(a).dtype, device="cuda")
    buf[skip:] = torch.from_numpy(a.reshape(-1).copy()).cuda()
    t = buf[skip:].view(a.shape)
    assert t.is_contiguous()
    return t


def main(tmp):
    assert torch.cuda.is_available()
    st = pu.Setup(tu.build_scene(os.path.join(tmp, "textures.glb")), SIDE, SIDE, max_depth=2)
    index = tu.texture_index(st.scene)
    rng = np.random.default_rng(40)
    u8, f32, chains8, chains32 = {}, {}, {}, {}
    for (w, h, srgb), i in sorted(index.items()):
        if (w, h) == tu.ALPHA_SIZE:
            continue
        u8[i] = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        chains8[i] = tu.host_chain(u8[i], srgb)
        img = rng.uniform(-0.1, 1.1, (h, w, 4)).astype(np.float32)
        img.reshape(-1)[::7] = np.float32(0.5) / np.float32(255.0) * rng.integers(0, 512, img.reshape(-1)[::7].size)
        img.reshape(-1)[3::11] = np.nan
        f32[i] = img
        chains32[i] = tu.host_chain(tu.host_quantise(img, srgb), srgb)
    rays, _ = tu.grid_rays([tu.SIZES.index((33, 17)), tu.SIZES.index((64, 16))], n=16)
    angle = tu.pixel_angle_for((33, 17), 2.5)

    host = tracer(st)
    host.update_textures(u8)
    want_img = view(host, st, rays, "BASE_COLOR", angle)
    host.close()

    dev = tracer(st)
    rest_img = view(dev, st, rays, "BASE_COLOR", angle)
    # uint8 tensors, some of them 4-byte but not 16-byte aligned: every level equals the host chain; nothing allocated stays
    t8 = {i: (offset_tensor(a, 4) if k % 2 else torch.from_numpy(a).cuda()) for k, (i, a) in enumerate(sorted(u8.items()))}
    torch.cuda.synchronize()
    dev.update_textures({sorted(t8)[0]: t8[sorted(t8)[0]]})  # (the tables are made by the first call)
    m0 = dev.memory()
    dev.update_textures(t8)
    m1 = dev.memory()
    assert all(m1[k] == m0[k] for k in ("sceneBytes", "rendererBytes", "pathStateBytes")), (m0, m1)
    for i in u8:
        assert same(chain(dev, st, i), chains8[i]), ("uint8", i)
    img = view(dev, st, rays, "BASE_COLOR", angle)
    assert img.tobytes() == want_img.tobytes() and img.tobytes() != rest_img.tobytes()
    # float32 tensors: the chain of the host-quantised level 0
    t32 = {i: torch.from_numpy(a).cuda() for i, a in f32.items()}
    torch.cuda.synchronize()
    dev.update_textures(t32)
    for i in f32:
        assert same(chain(dev, st, i), chains32[i]), ("float32", i)
    info = dev.texture_update_info()
    assert info["calls"] == 3 and info["levelsGenerated"] == 2 * sum(len(c) - 1 for c in chains8.values()) + len(chains8[sorted(t8)[0]]) - 1, info
    # a complete chain of device tensors
    some = sorted(u8)[-2:]
    dev.update_textures({i: [torch.from_numpy(l).cuda() for l in chains8[i]] for i in some}, generate_mips=False)
    for i in f32:
        assert same(chain(dev, st, i), chains8[i] if i in some else chains32[i]), ("chain", i)

    # numpy arrays and tensors in one call, a tensor of another type, a strided one, a host tensor: refused by the binding
    a, b = sorted(u8)[-1], sorted(u8)[-3]
    for bad in ({a: t8[a], b: u8[b]}, {a: t8[a].double()}, {a: t8[a][:, ::2]}, {a: t8[a].to(torch.int32)}):
        try:
            dev.update_textures(bad)
            raise SystemExit("a bad update was accepted: %r" % ({k: type(v) for k, v in bad.items()},))
        except ValueError:
            pass
    # misaligned device pointers: uint8 texels off a 4-byte boundary, float texels off a 16-byte one -- refused by the library, nothing changes
    before = [l.tobytes() for i in sorted(u8) for l in chain(dev, st, i)]
    for bad in ({a: offset_tensor(u8[a], 2)}, {a: offset_tensor(f32[a], 2)}):
        assert next(iter(bad.values())).data_ptr() % (4 if next(iter(bad.values())).dtype == torch.uint8 else 16) != 0
        try:
            dev.update_textures(bad)
            raise SystemExit("a misaligned pointer was accepted")
        except ptmod.MiError as e:
            assert "rc=-1" in str(e) and "aligned" in str(e), str(e)
    assert [l.tobytes() for i in sorted(u8) for l in chain(dev, st, i)] == before
    dev.close()
    print("TEXTURE_UPDATE_DEVICE_OK")


if __name__ == "__main__":
    main(sys.argv[1])
