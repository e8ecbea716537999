"""Skins and morph targets on the device (csrc/device/deform.hip through mi_pt_set_deformation / mi_pt_update_deformation): the kernel's
vertices against the two shaders restated in float32 numpy (tests/deform_util.py), the posed render against a fresh instance created from
the read-back vertices (bit for bit), against the host deformation and the CPU oracle, one rebuild per animated frame, constant memory,
queued frames, and scenes without deformers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import deform_util as du
import parity_util as pu
from vk_gltf_renderer_amd import pathtracer as ptmod
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 128, 96, 2


@pytest.fixture(scope="module")
def skinned(tmp_path_factory):
    return scenegen.scene_skinned(str(tmp_path_factory.mktemp("gpu_deform") / "skinned.glb"))


def _tracer(st):
    tr = ptmod.PathTracer(st.scene)
    tr.resize(st.width, st.height)
    tr.set_frame_info(st.frame_info)
    tr.set_sky(st.sky)
    return tr


def _render(tr, st, frames=FRAMES):
    total = 0
    for f in range(frames):
        p = st.frame_params(f, total)
        tr.render_frame(p)
        total += p.numSamples
    return tr.read_accum()


def test_kernel_matches_the_shaders(skinned):
    st = pu.Setup(skinned, W, H, max_depth=3)
    tr = _tracer(st)
    tr.set_deformation(st.scene)
    d = st.scene.deformation
    kinds = set()
    for time in (0.0, 0.9, 1.6, 2.4):
        st.scene.update_animation(0, time)
        jt, mw = du.frame_tables(d)
        tr.update_deformation(d.jointMatrices, d.morphWeights)
        for p in du.prims(d):
            ep, en, et = du.deform_reference(p, jt, mw, np.float32)
            gp, gn, gt = tr.read_vertices(p.renderPrimID)
            ext = max(1.0, float(np.abs(ep).max()))
            assert np.abs(gp - ep).max() <= 1e-6 * ext, (time, p.renderPrimID, np.abs(gp - ep).max())
            if en is not None:
                assert np.abs(gn - en).max() <= 2e-6, (time, p.renderPrimID, np.abs(gn - en).max())
            if et is not None:
                assert np.abs(gt[:, :3] - et[:, :3]).max() <= 2e-6, (time, p.renderPrimID, np.abs(gt[:, :3] - et[:, :3]).max())
                assert np.array_equal(gt[:, 3].view(np.uint32), du.arr(p.baseTangents, p.vertexCount * 4).reshape(-1, 4)[:, 3].view(np.uint32))
            kinds.add((bool(p.joints), p.numTargets > 0))
            if time == 0.0 and p.numTargets == 3:  # the blob's weights are all zero: its positions stay bit for bit
                assert not mw[p.morphWeightOffset:p.morphWeightOffset + 3].any()
                assert np.array_equal(gp.reshape(-1).view(np.uint32), du.arr(p.basePositions, p.vertexCount * 3).view(np.uint32))
    assert kinds == {(True, False), (False, True), (True, True)}
    tr.close()


def test_posed_render_is_a_fresh_instance_of_the_posed_vertices(skinned):
    st = pu.Setup(skinned, W, H, max_depth=3)
    tr = _tracer(st)
    tr.set_deformation(st.scene)
    rest = _render(tr, st)
    d = st.scene.deformation
    for time in (0.6, 1.4, 2.7):
        assert st.scene.update_animation(0, time)
        tr.update_from_scene(st.scene)
        moved = _render(tr, st)
        sel = tr.read_selection()
        streams = {p.renderPrimID: tr.read_vertices(p.renderPrimID) for p in du.prims(d)}
        holder, keep = du.posed_desc(st.scene, streams)
        fresh = ptmod.PathTracer(holder)
        fresh.resize(W, H)
        fresh.set_frame_info(st.frame_info)
        fresh.set_sky(st.sky)
        img = _render(fresh, st)
        assert (moved == img).all(), time
        assert (sel == fresh.read_selection()).all(), time
        fresh.close()
        assert not (moved == rest).all()
        # the same pose deformed on the host: a fresh instance of it, and the oracle
        hs = pu.Setup(skinned, W, H, max_depth=3)
        assert hs.scene.update_animation(0, time)
        assert hs.scene.deform_on_host() == d.numPrims
        host = pu.render_gpu(hs, FRAMES, collect_counters=False)
        cmp = pu.compare_images(host["accum"], moved)
        assert cmp["rel_l2"] < 5e-3 and (host["selection"] == sel).mean() >= 0.999, (time, cmp)
        if time == 1.4:
            ref = pu.render_oracle(hs, FRAMES)
            cmp = pu.compare_images(ref["accum"], moved)
            print("deformed pose vs oracle", cmp)
            assert cmp["rel_l2"] < 5e-3 and (ref["selection"] == sel).mean() >= 0.999, cmp
    tr.close()


def test_one_rebuild_per_animated_frame(skinned):
    """MI_PT_BUILD_TIMING prints one "deform" and one "rebuild" line per animated frame of update_from_scene (deferred build), and one
    of each for a plain update_deformation."""
    script = (
        "import sys; sys.path[:0] = [%r, %r]\n"
        "import parity_util as pu\n"
        "from vk_gltf_renderer_amd import pathtracer as ptmod\n"
        "st = pu.Setup(%r, 64, 48, max_depth=2)\n"
        "tr = ptmod.PathTracer(st.scene)\n"
        "tr.set_deformation(st.scene)\n"
        "print('[mark] animated', file=sys.stderr, flush=True)\n"
        "for t in (0.5, 1.5, 2.5):\n"
        "    st.scene.update_animation(0, t)\n"
        "    tr.update_from_scene(st.scene)\n"
        "print('[mark] single', file=sys.stderr, flush=True)\n"
        "d = st.scene.deformation\n"
        "tr.update_deformation(d.jointMatrices, d.morphWeights)\n"
        "tr.close()\n") % (ROOT, os.path.join(ROOT, "tests"), skinned)
    env = dict(os.environ, MI_PT_BUILD_TIMING="1")
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    log = r.stderr.split("[mark] animated")[1]
    animated, single = log.split("[mark] single")

    def count(text, what):
        return sum(1 for line in text.splitlines() if line.startswith("[mi_pt build]") and line.split()[2] == what)
    assert count(animated, "deform") == 3 and count(animated, "rebuild") == 3, animated
    assert count(single, "deform") == 1 and count(single, "rebuild") == 1, single


def test_updates_do_not_leak_and_queued_frames_keep_the_old_pose(skinned):
    st = pu.Setup(skinned, W, H, max_depth=3)
    tr = _tracer(st)
    before = tr.memory()["sceneBytes"]
    tr.set_deformation(st.scene)
    with_tables = tr.memory()["sceneBytes"]
    assert with_tables > before
    # (sceneBytes includes the acceleration structure, whose size follows the pose: alternate two poses, the bytes must repeat)
    seen = []
    for k in range(20):
        st.scene.update_animation(0, (0.4, 1.9)[k % 2])
        tr.update_from_scene(st.scene)
        seen.append(tr.memory()["sceneBytes"])
        assert k < 2 or seen[k] == seen[k - 2], (k, seen)
    tr.set_deformation(None)
    st.scene.update_animation(0, 1.9)
    tr.update_from_scene(st.scene)  # (no deformation any more: the pose stays, the tables are gone)
    assert tr.memory()["sceneBytes"] == seen[-1] - (with_tables - before)
    tr.close()

    # frames queued before an update are rendered with the pose they were queued under
    ref_st = pu.Setup(skinned, W, H, max_depth=3)
    ref = _tracer(ref_st)
    want = _render(ref, ref_st, 3)  # rest pose, depth 1
    ref.close()
    q_st = pu.Setup(skinned, W, H, max_depth=3)
    q = _tracer(q_st)
    q.set_deformation(q_st.scene)
    q.set_frame_queue(8)
    total = 0
    for f in range(3):
        p = q_st.frame_params(f, total)
        q.render_frame(p)
        total += p.numSamples
    q_st.scene.update_animation(0, 1.1)
    q.update_from_scene(q_st.scene)  # flushes the three queued frames first
    assert (q.read_accum() == want).all()
    q.close()


def test_a_scene_without_deformers_renders_as_before(assets):
    st = pu.Setup(os.path.join(assets, "Box.glb"), W, H, max_depth=3)
    want = pu.render_gpu(st, FRAMES, collect_counters=False)["accum"]
    tr = _tracer(st)
    tr.set_deformation(None)
    tr.set_deformation(st.scene)  # (nothing to deform: releases / allocates nothing)
    assert st.scene.deformation is None
    before = tr.memory()["sceneBytes"]
    tr.update_from_scene(st.scene)
    assert (_render(tr, st) == want).all()
    assert tr.memory()["sceneBytes"] == before
    tr.close()
