"""mi_camera_rays (include/mi_host.h, csrc/host/mi_host.cpp; CPU only) against float64 numpy restatements of its three projections, written from
the formulas in the header: every origin and direction component within one float32 unit in the last place of the float64 value rounded to
float32 (the helper computes in double and rounds once; the restatement's own double arithmetic may differ from it in the last double place,
which moves a rounding to float32 by at most one unit).  A perspective and an orthographic camera, 9 x 5 and 64 x 32."""
import numpy as np
import pytest

from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

F32 = np.float32
SIZES = [(9, 5), (64, 32)]
JITTER = np.asarray([(0.5, 0.5), (0.125, 0.875), (0.99, 0.01)], F32)


def camera(kind):
    cam = capi.MiCamera()
    cam.eye[:] = [1.5, 2.25, 4.0]
    cam.center[:] = [0.25, 0.5, -0.75]
    cam.up[:] = [0.0, 1.0, 0.0]
    cam.fovDegrees, cam.znear, cam.zfar = 47.0, 0.1, 100.0
    if kind == "orthographic":
        cam.orthographic, cam.xmag, cam.ymag = 1, 3.0, 2.0
    return cam


def frame(cam, w, h):
    fi, angle, _ = ptmod.camera_frame_info(cam, w, h)
    V = np.array(fi.viewInv[:], np.float64).reshape(4, 4).T  # column-major storage -> V[row, column]
    Pi = np.array(fi.projInv[:], np.float64).reshape(4, 4).T
    return V, Pi, angle, V[:3, 0], V[:3, 1], -V[:3, 2], V[:3, 3]


def samples(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (xs[None] + JITTER[:, 0].astype(np.float64)[:, None, None]), (ys[None] + JITTER[:, 1].astype(np.float64)[:, None, None])


def unit(d):
    n = np.linalg.norm(d, axis=-1, keepdims=True)
    return np.where(n > 0, d / np.where(n > 0, n, 1), 0)


def within_one_ulp(got, want64):
    want = want64.astype(F32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)


def check(rays, origin64, dir64, w, h):
    assert rays.shape == (len(JITTER), h, w, 8) and rays.dtype == F32
    assert (rays[..., 3] == 0).all() and (rays[..., 7] == np.finfo(F32).max).all()  # a valid query input
    assert within_one_ulp(rays[..., :3], np.broadcast_to(origin64, rays[..., :3].shape)).all()
    assert within_one_ulp(rays[..., 4:7], dir64).all()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
def test_perspective_is_the_builtin_camera_without_its_lens(kind, w, h):
    cam = camera(kind)
    V, Pi, angle, right, up, forward, eye = frame(cam, w, h)
    x, y = samples(w, h)
    clip = np.stack([x / w * 2 - 1, y / h * 2 - 1, -np.ones_like(x), np.ones_like(x)], -1)
    view = clip @ Pi.T
    view = view / view[..., 3:4]
    world = view @ V.T
    if kind == "orthographic":
        origin, d = world[..., :3], np.broadcast_to(V @ np.array([0.0, 0, -1, 0]), world.shape)[..., :3]
    else:
        origin, d = eye, world[..., :3] - eye
    rays, pa = ptmod.camera_rays(cam, w, h, "perspective", jitter=JITTER)
    check(rays, origin, unit(d), w, h)
    assert pa == angle  # mi_camera_frame_info's
    centre = ptmod.camera_rays(cam, w, h, "perspective")[0]
    assert centre.shape == (1, h, w, 8) and (centre[0] == rays[0]).all()  # no jitter: the pixel centres


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
def test_equirect(kind, w, h):
    cam = camera(kind)
    V, _, _, right, up, forward, eye = frame(cam, w, h)
    x, y = samples(w, h)
    phi, theta = (x / w - 0.5) * 2 * np.pi, (0.5 - y / h) * np.pi
    d = (np.cos(theta) * np.sin(phi))[..., None] * right + np.sin(theta)[..., None] * up + (np.cos(theta) * np.cos(phi))[..., None] * forward
    rays, pa = ptmod.camera_rays(cam, w, h, "equirect", jitter=JITTER)
    check(rays, eye, unit(d), w, h)
    assert pa == F32(np.pi / h)
    # the centre sample looks along `forward`; row 0 is the top row
    mid = ptmod.camera_rays(cam, w, h, "equirect", jitter=[(w / 2 - w // 2, h / 2 - h // 2)])[0][0, h // 2, w // 2, 4:7]
    assert within_one_ulp(mid, unit(forward)).all()
    dots = rays[0, ..., 4:7].astype(np.float64) @ up
    assert (dots[0] > dots[-1]).all() and (np.diff(dots, axis=0) < 0).all()


@pytest.mark.parametrize("fov", [180.0, 360.0, 97.5])
@pytest.mark.parametrize("w,h", SIZES)
def test_fisheye(w, h, fov):
    cam = camera("perspective")
    V, _, _, right, up, forward, eye = frame(cam, w, h)
    x, y = samples(w, h)
    R = min(w, h) / 2
    u, v = (x - w / 2) / R, (h / 2 - y) / R
    r = np.sqrt(u * u + v * v)
    alpha = r * np.radians(np.float64(F32(fov))) / 2
    rs = np.where(r > 0, r, 1)
    d = (np.sin(alpha) / rs)[..., None] * (u[..., None] * right + v[..., None] * up) + np.cos(alpha)[..., None] * forward
    d = np.where((r > 1)[..., None], 0.0, unit(d))
    rays, pa = ptmod.camera_rays(cam, w, h, "fisheye", fov=fov, jitter=JITTER)
    check(rays, eye, d, w, h)
    dead = (rays[..., 4:7] == 0).all(-1)
    assert (dead == (r > 1)).all() and dead.any() and not dead.all()  # dead exactly outside the image circle
    assert pa == F32(np.radians(np.float64(F32(fov))) / min(w, h))
    if fov == 360.0:  # the rim looks backwards
        rim = (r > 0.97) & (r <= 1)
        assert rim.any() and (rays[..., 4:7].astype(np.float64)[rim] @ forward < -0.98).all()


def test_argument_errors():
    cam = camera("perspective")
    L = capi.host_lib()
    rays = np.zeros((1, 5, 9, 8), F32)
    ptr = rays.ctypes.data_as(capi.P(capi.MiPtRay))
    assert L.mi_camera_rays(cam, 1, 180.0, 9, 5, None, 1, ptr, None) == 0 and (rays[..., 4:7] != 0).any()
    for args in ((None, 1, 180.0, 9, 5, None, 1, ptr, None), (cam, 3, 180.0, 9, 5, None, 1, ptr, None), (cam, 1, 180.0, 0, 5, None, 1, ptr, None),
                 (cam, 1, 180.0, 9, 5, None, 0, ptr, None), (cam, 1, 180.0, 9, 5, None, 1, None, None), (cam, 2, 0.0, 9, 5, None, 1, ptr, None),
                 (cam, 2, 361.0, 9, 5, None, 1, ptr, None), (cam, 2, float("nan"), 9, 5, None, 1, ptr, None)):
        assert L.mi_camera_rays(*args) == -1, args
    with pytest.raises(KeyError):
        ptmod.camera_rays(cam, 9, 5, "cylinder")
