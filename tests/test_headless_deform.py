"""The headless app plays skinned and morphed clips (csrc/app/renderer.cpp: updateAnimation uploads the skin / morph tables once and deforms
every animated frame before the render-node update): --animTime on scenegen.scene_skinned writes the image of the Python path on the same
pose and frame schedule, and it differs from the rest pose."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vk_gltf_renderer_amd", "lib", "mi_gltf_renderer")


@pytest.mark.gpu
def test_anim_time_poses_skinned_scene(tmp_path, assets):
    import parity_util as pu
    from vk_gltf_renderer_amd import pathtracer as ptmod
    from vk_gltf_renderer_amd import scenegen
    glb = scenegen.scene_skinned(str(tmp_path / "skinned.glb"))
    hdr = os.path.join(assets, "std_env.hdr")
    common = [APP, "--headless", "--size", "160", "96", "--scenefile", glb, "--hdrfile", hdr, "--ptSamples", "1", "--ptAdaptiveSampling", "0",
              "--envSystem", "1", "--ptMaxDepth", "3", "--frames", "4", "--maxFrames", "4"]

    def run(extra, out):
        r = subprocess.run(common + extra + ["--output", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        h = ptmod.HdrEnvironment(path=str(out))
        e = h.env.contents
        return np.ctypeslib.as_array(e.rgba, shape=(e.height, e.width, 4))[..., :3].copy()

    posed = run(["--animTime", "1.4"], tmp_path / "posed.hdr")
    rest = run([], tmp_path / "rest.hdr")

    st = pu.Setup(glb, 160, 96, hdr_path=hdr, max_depth=3)
    tr = ptmod.PathTracer(st.scene)
    tr.set_environment(st.hdr)
    tr.resize(160, 96)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    tr.set_deformation(st.scene)
    assert st.scene.update_animation(0, 1.4)
    tr.update_from_scene(st.scene)
    total = 0
    for f in range(4):
        p = st.frame_params(f, total)
        tr.render_frame(p)
        total += p.numSamples
    want = tr.read_accum()[..., :3]
    tr.close()
    assert np.abs(posed - want).max() <= want.max() / 128 + 1e-3  # (the .hdr file is RGBE: 8-bit mantissas)
    assert np.abs(rest - want).max() > 0.05
