"""The headless app plays KHR_animation_pointer clips (csrc/app/renderer.cpp: updateAnimation hands the material tables to
mi_pt_update_materials when a channel changed them, and takes the animated camera's projection): --animTime on
scenegen.scene_material_animated at two times writes two different images, each the image of the Python path at that time."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vk_gltf_renderer_amd", "lib", "mi_gltf_renderer")


@pytest.mark.gpu
def test_anim_time_poses_materials_lights_camera_and_visibility(tmp_path, assets):
    import parity_util as pu
    from vk_gltf_renderer_amd import _capi as capi
    from vk_gltf_renderer_amd import pathtracer as ptmod
    from vk_gltf_renderer_amd import scenegen
    glb = scenegen.scene_material_animated(str(tmp_path / "stage.glb"))
    hdr = os.path.join(assets, "std_env.hdr")
    common = [APP, "--headless", "--size", "160", "96", "--scenefile", glb, "--hdrfile", hdr, "--ptSamples", "1", "--ptAdaptiveSampling", "0",
              "--envSystem", "1", "--ptMaxDepth", "4", "--frames", "4", "--maxFrames", "4"]

    def run(time, out):
        r = subprocess.run(common + ["--animTime", str(time), "--output", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        h = ptmod.HdrEnvironment(path=str(out))
        e = h.env.contents
        return np.ctypeslib.as_array(e.rgba, shape=(e.height, e.width, 4))[..., :3].copy()

    def python_path(time):
        st = pu.Setup(glb, 160, 96, hdr_path=hdr, max_depth=4)
        tr = ptmod.PathTracer(st.scene)
        tr.set_environment(st.hdr)
        tr.resize(160, 96)
        tr.set_sky(st.sky)
        assert st.scene.update_animation(0, time)
        assert st.scene.animation_changes & capi.MI_SCENE_CHANGED_MATERIALS
        fi, st.params.pixelAngle, st.params.focalDistance = ptmod.camera_frame_info(st.scene.camera(0), 160, 96)  # (the yfov channel)
        fi.flags |= capi.MI_SCENE_USE_HDR_ENVIRONMENT
        tr.set_frame_info(fi)
        tr.update_from_scene(st.scene)
        total = 0
        for f in range(4):
            p = st.frame_params(f, total)
            tr.render_frame(p)
            total += p.numSamples
        img = tr.read_accum()[..., :3]
        tr.close()
        return img

    images = {}
    for time in (0.9, 1.5):
        images[time] = run(time, tmp_path / ("t%s.hdr" % time))
        want = python_path(time)
        assert np.abs(images[time] - want).max() <= want.max() / 128 + 1e-3, time  # (the .hdr file is RGBE: 8-bit mantissas)
    assert np.abs(images[0.9] - images[1.5]).max() > 0.05
