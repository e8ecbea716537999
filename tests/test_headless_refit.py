"""The headless app's --accelUpdate / --accelRebuildRatio (csrc/app/renderer_pathtracer.cpp: mi_pt_set_accel_update right after mi_pt_create):
a played clip (--animStep) writes the same output file whether its animated frames rebuild the BVH or refit it, for a node-transform clip
and a skinned one; an unknown mode or a ratio below 1 is reported."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "vk_gltf_renderer_amd", "lib", "mi_gltf_renderer")


def _run(args):
    return subprocess.run([APP] + args, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["animated", "skinned"])
def test_refit_playback_writes_the_rebuild_playbacks_file(tmp_path, assets, kind):
    from vk_gltf_renderer_amd import scenegen
    glb = getattr(scenegen, "scene_" + kind)(str(tmp_path / (kind + ".glb")))
    hdr = os.path.join(assets, "std_env.hdr")
    common = ["--headless", "--size", "160", "96", "--scenefile", glb, "--hdrfile", hdr, "--ptSamples", "1", "--ptAdaptiveSampling", "0",
              "--envSystem", "1", "--ptMaxDepth", "4", "--frames", "5", "--maxFrames", "100", "--animStep", "0.25"]
    files = {}
    for mode, extra in (("0", []), ("1", []), ("2", ["--accelRebuildRatio", "1.2"])):
        out = tmp_path / ("play_%s.hdr" % mode)
        r = _run(common + ["--accelUpdate", mode] + extra + ["--output", str(out)])
        assert r.returncode == 0, r.stdout + r.stderr
        files[mode] = out.read_bytes()
    assert files["1"] == files["0"] and files["2"] == files["0"]


@pytest.mark.gpu
def test_bad_accel_switches_are_reported(tmp_path, assets):
    from vk_gltf_renderer_amd import scenegen
    glb = scenegen.scene_animated(str(tmp_path / "animated.glb"))
    common = ["--headless", "--size", "64", "48", "--scenefile", glb, "--ptSamples", "1", "--frames", "1", "--maxFrames", "1"]
    for extra in (["--accelUpdate", "3"], ["--accelUpdate", "2", "--accelRebuildRatio", "0.5"]):
        r = _run(common + extra + ["--output", str(tmp_path / "x.hdr")])
        assert "mi_pt_set_accel_update failed" in r.stderr, r.stdout + r.stderr
