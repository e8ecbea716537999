"""The a-trous denoiser (SURVEY §8f.1, I/O contract of the reference's OptiX adapter: src/optix_denoiser.hpp:128-153) against
a numpy restatement of the same filter on the same inputs, plus the properties a denoiser must have."""
import os

import numpy as np
import pytest

import parity_util as pu
from denoise_ref import _atrous_numpy, _svgf_numpy
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

pytestmark = pytest.mark.gpu


def test_atrous_matches_numpy_and_reduces_noise(built, assets):
    hdr = os.path.join(assets, "std_env.hdr")
    s = pu.Setup(os.path.join(assets, "shader_ball.gltf"), 160, 120, max_depth=5, hdr_path=hdr,
                 params_edit=lambda p: setattr(p, "flags", p.flags | capi.MI_PT_USE_OPTIX_DENOISER))
    tracer = ptmod.PathTracer(s.scene)
    try:
        tracer.set_environment(s.hdr)
        tracer.resize(s.width, s.height)
        tracer.set_frame_info(s.frame_info)
        tracer.set_sky(s.sky)
        total = 0
        for f in range(4):
            p = s.frame_params(f, total)
            tracer.render_frame(p)
            total += p.numSamples
        noisy = tracer.read_accum()
        albedo, normal = tracer.read_guides()
        den = tracer.denoise(iterations=4, sigma_color=3.0, sigma_normal=64.0, sigma_albedo=0.2)
        # a converged reference of the same view
        for f in range(4, 260):
            p = s.frame_params(f, total)
            tracer.render_frame(p)
            total += p.numSamples
        ref = tracer.read_accum()
    finally:
        tracer.close()
    # guides: albedo.w is the first-hit fraction; normals are means of unit vectors over the samples that hit
    hit = albedo[..., 3] > 0.5
    assert 0.05 < hit.mean() < 0.95
    nlen = np.linalg.norm(normal[hit][:, :3], axis=1)
    assert nlen.max() <= 1.0 + 1e-3 and nlen.mean() > 0.85
    want = _atrous_numpy(noisy, albedo, normal, 4, 3.0, 64.0, 0.2)
    # the device uses the fast exp/pow intrinsics: compare with a tolerance relative to the image scale
    scale = np.abs(want[..., :3]).mean()
    assert np.abs(den[..., :3] - want[..., :3]).max() <= 2e-2 * scale + 1e-3 * np.abs(want[..., :3]).max()
    assert np.array_equal(den[..., 3], noisy[..., 3])
    # and it denoises: closer to the converged image than the 4-spp input on the geometry
    err_noisy = np.sqrt(((noisy[hit][:, :3] - ref[hit][:, :3]) ** 2).mean())
    err_den = np.sqrt(((den[hit][:, :3] - ref[hit][:, :3]) ** 2).mean())
    assert err_den < 0.85 * err_noisy, (err_den, err_noisy)


@pytest.mark.parametrize("frames", [2, 16])
def test_svgf_matches_numpy_and_beats_plain_atrous(built, assets, frames):
    """Variance-guided pass: numpy parity on the same inputs (temporal variance at 16 frames, the spatial fallback at 2), the second
    moment really is E[l^2] of the per-frame luminance, and on equal inputs it ends closer to the converged image than the 4-spp input."""
    hdr = os.path.join(assets, "std_env.hdr")
    s = pu.Setup(os.path.join(assets, "shader_ball.gltf"), 160, 120, max_depth=5, hdr_path=hdr,
                 params_edit=lambda p: setattr(p, "flags", p.flags | capi.MI_PT_USE_OPTIX_DENOISER))
    tracer = ptmod.PathTracer(s.scene)
    try:
        tracer.set_environment(s.hdr)
        tracer.resize(s.width, s.height)
        tracer.set_frame_info(s.frame_info)
        tracer.set_sky(s.sky)
        total, lum2 = 0, np.zeros((s.height, s.width))
        for f in range(frames):
            p = s.frame_params(f, total)
            tracer.render_frame(p)
            total += p.numSamples
            if frames <= 16:  # per-frame pixel value from consecutive running means (float64: exact enough for a 1e-3 check)
                cur = tracer.read_accum().astype(np.float64)
                frame_px = cur * (f + 1) - prev * f if f else cur
                prev = cur
                lum2 += (frame_px[..., :3] @ np.array([0.2126, 0.7152, 0.0722])) ** 2
        noisy = tracer.read_accum()
        albedo, normal = tracer.read_guides()
        depth = tracer.read_depth()
        den = tracer.denoise_svgf(iterations=4, sigma_luminance=4.0, sigma_normal=64.0, sigma_depth=1.0)
        den_dev = tracer.tonemap(source=1, method="clip")  # the denoised image is routed to the tonemapper like the OptiX output
        for f in range(frames, 300):
            p = s.frame_params(f, total)
            tracer.render_frame(p)
            total += p.numSamples
        ref = tracer.read_accum()
    finally:
        tracer.close()
    m2 = lum2 / frames
    assert np.abs(normal[..., 3] - m2).max() <= 2e-3 * max(1.0, m2.max())
    want = _svgf_numpy(noisy, albedo, normal, depth, frames, 4, 4.0, 64.0, 1.0)
    scale = np.abs(want[..., :3]).mean()
    err = np.abs(den[..., :3] - want[..., :3])
    assert np.quantile(err, 0.999) <= 2e-3 * scale and err.max() <= 5e-2 * np.abs(want[..., :3]).max(), (np.quantile(err, 0.999), err.max(), scale)
    assert np.array_equal(den[..., 3], noisy[..., 3])
    srgb = np.where(den[..., :3] > 0.0031308, 1.055 * np.maximum(den[..., :3], 1e-30) ** (1 / 2.4) - 0.055, 12.92 * den[..., :3])
    assert np.abs(den_dev[..., :3].astype(np.float64) - np.clip(srgb, 0, 1) * 255.0).max() <= 0.51
    hit = albedo[..., 3] > 0.5
    err_noisy = np.sqrt(((noisy[hit][:, :3] - ref[hit][:, :3]) ** 2).mean())
    err_den = np.sqrt(((den[hit][:, :3] - ref[hit][:, :3]) ** 2).mean())
    assert err_den < 0.8 * err_noisy, (err_den, err_noisy)
