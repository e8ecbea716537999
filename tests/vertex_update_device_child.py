"""Child process of tests/test_gpu_vertex_update.py::test_device_form_with_torch_tensors: the device form of the vertex updates
(mi_pt_update_vertices_device) fed with torch tensors.  torch is imported BEFORE libmi_pt.so is loaded, so that both use the one HIP runtime
torch brings.
usage: python tests/vertex_update_device_child.py <scratch directory>"""
import os
import sys

import torch  # (first: see above)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import deform_util as du  # noqa: E402
import parity_util as pu  # noqa: E402
import vertex_update_util as vu  # noqa: E402
from vk_gltf_renderer_amd import pathtracer as ptmod  # noqa: E402
from vk_gltf_renderer_amd import scenegen  # noqa: E402

W, H, FRAMES = 128, 96, 2
CLOTH, BALL, BOX, TRIANGLE = 336, 325, 24, 3


def tracer(st, scene=None):
    tr = ptmod.PathTracer(scene if scene is not None else st.scene)
    tr.resize(W, H)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    return tr


def render(tr, st):
    total = 0
    for f in range(FRAMES):
        p = st.frame_params(f, total)
        tr.render_frame(p)
        total += p.numSamples
    return tr.read_accum()


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def offset_tensor(a):
    """The array as a contiguous device tensor that starts one float into its allocation: 4-byte aligned, not 16."""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(a.reshape(-1).copy()).cuda()
    t = buf[1:].view(a.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def main(tmp):
    assert torch.cuda.is_available()
    st = pu.Setup(scenegen.scene_dynamic(os.path.join(tmp, "dynamic.glb")), W, H, max_depth=3)
    d = st.scene.desc.contents
    ids = {int(d.renderPrimitives[i].vertexCount): i for i in range(int(d.numRenderPrimitives))}
    cloth, ball, box, tri = ids[CLOTH], ids[BALL], ids[BOX], ids[TRIANGLE]
    host = tracer(st)
    host.set_vertex_updates([cloth, ball, box, tri], recompute_normals=True)
    rest = {p: host.read_vertices(p) for p in (cloth, ball, box, tri)}
    cp, cn, ct = vu.cloth_wave(rest[cloth][0], 1.1)
    pose = {cloth: (cp, cn, ct), ball: vu.ball_pulse(rest[ball][0], rest[ball][1], 0.6)[0],  # (the ball's normals are rebuilt)
            box: (vu.box_shear(rest[box][0], 0.4), None, None), tri: vu.triangle_move(rest[tri][0], (0.1, 0.2, -0.1))}
    host.update_vertices(pose)
    want = {p: host.read_vertices(p) for p in pose}
    want_img, want_sel = render(host, st), host.read_selection()
    host.close()

    # torch tensors in: streams and image equal the host form's bit for bit, and the call allocates nothing
    dev = tracer(st)
    dev.set_accel_update("refit")
    dev.set_vertex_updates([cloth, ball, box, tri], recompute_normals=True)
    rest_img = render(dev, st)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tensors = {cloth: (offset_tensor(cp), up(cn), offset_tensor(ct)), ball: up(pose[ball]), box: (up(pose[box][0]), None, None), tri: offset_tensor(pose[tri])}
    torch.cuda.synchronize()
    m0, a0 = dev.memory(), dev.accel_info()
    dev.update_vertices(tensors)
    m1, a1 = dev.memory(), dev.accel_info()
    assert all(m1[k] == m0[k] for k in ("sceneBytes", "rendererBytes", "pathStateBytes")), (m0, m1)
    assert a1["refits"] == a0["refits"] + 1 and a1["builds"] == a0["builds"], (a0, a1)
    info = dev.vertex_update_info()
    assert info["calls"] == 1 and info["verticesRejected"] == 0 and info["verticesWritten"] == CLOTH + BALL + BOX + TRIANGLE, info
    for p in pose:
        got = dev.read_vertices(p)
        assert all((g is None and w is None) or same(g, w) for g, w in zip(got, want[p])), p
    img = render(dev, st)
    assert (img == want_img).all() and (dev.read_selection() == want_sel).all() and not (img == rest_img).all()

    # numpy arrays and tensors in one call, a tensor of another type, a strided one: refused by the binding
    for bad in ({cloth: (up(cp), cn, None)}, {cloth: up(cp).double()}, {cloth: up(np.zeros((CLOTH, 6), np.float32))[:, :3]},
                {cloth: torch.from_numpy(cp.copy())}):
        try:
            dev.update_vertices(bad)
            raise SystemExit("a bad update was accepted: %r" % ({k: type(v) for k, v in bad.items()},))
        except ValueError:
            pass

    # 5 non-finite vertices among 336 -- the first and last lane of a wave, the last of the full block, the last of the partial one, one inside:
    # exactly those keep ALL their resident values, the others are written; the refit and the render that follow are finite
    before = dev.read_vertices(cloth)
    np2, nn2, nt2 = vu.cloth_wave(rest[cloth][0], 2.6)
    salted = [np2.copy(), nn2.copy(), nt2.copy()]
    bad = {0: (0, 0, np.nan), 63: (0, 2, np.inf), 100: (1, 1, -np.inf), 255: (2, 3, np.nan), 335: (2, 0, np.inf)}
    for v, (stream, c, value) in bad.items():
        salted[stream][v, c] = value
    a0 = dev.accel_info()
    dev.update_vertices({cloth: tuple(up(a) for a in salted)})
    info, a1 = dev.vertex_update_info(), dev.accel_info()
    assert info["verticesRejected"] == 5 and info["calls"] == 2 and info["verticesWritten"] == CLOTH + BALL + BOX + TRIANGLE + CLOTH - 5, info
    assert a1["refits"] == a0["refits"] + 1 and np.isfinite(a1["sahCost"]) and a1["sahCost"] > 0, (a0, a1)
    after = dev.read_vertices(cloth)
    keep = np.zeros(CLOTH, bool)
    keep[list(bad)] = True
    for got, old, new in zip(after, before, (np2, nn2, nt2)):
        assert np.isfinite(got).all() and same(got[keep], old[keep]) and same(got[~keep], new[~keep])
    img = render(dev, st)
    assert np.isfinite(img).all() and img[..., :3].max() > 0
    holder, keep_alive = du.posed_desc(st.scene, {p: dev.read_vertices(p) for p in pose})
    fresh = tracer(st, holder)
    assert (render(fresh, st) == img).all()
    fresh.close()
    # a clean call afterwards reports no rejection
    dev.update_vertices({tri: up(pose[tri])})
    assert dev.vertex_update_info()["verticesRejected"] == 0
    dev.close()
    del keep_alive
    print("VERTEX_UPDATE_DEVICE_OK")


if __name__ == "__main__":
    main(sys.argv[1])
