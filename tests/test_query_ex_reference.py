"""The yardstick of tests/test_gpu_query_ex.py, checked without a GPU: on the four scenes and the ray recipe of that test (query_ex_util.SCENES,
make_rays_ex) the float64 reference of the alpha-aware and face-culled queries marks at most 2 % of the rays of every single-hit comparison
ambiguous, and both alpha outcomes -- a tested candidate rejected, a tested candidate accepted -- occur on at least 5 % of the rays; the float32
ray / triangle test differs from float64 on the two zoo scenes by what query_ex_util.MEASURED records; and the device's own per-ray code
(csrc/device/pt_query.h through tests/host_shim/query_ex_on_host.cpp), run over every triangle instead of a tree, passes the very checks the GPU
records must pass: query_util.check_hits for the single-hit modes, query_ex_util.check_lists for the K nearest.

Measured here (2048 rays per scene; ambiguous shares of CUTOFF 0.5 / CUTOFF 0.9 / STOCHASTIC seed 1 / seed 99 / CULL_MATERIAL / CUTOFF + CULL;
rays with a rejected / an accepted tested candidate under CUTOFF 0.5):
  mixed alpha + glass  2 508 triangles  0.05 0.00 0.00 0.00 0.00 0.05 %   138 / 1 050
  zoo "blend"          3 136            0.05 0.00 0.05 0.05 0.00 0.00 %   896 /   472
  zoo "vertex_streams" 3 136            0.00 0.00 0.00 0.00 0.05 0.00 %   634 /   777
  sliver atrium       31 792            0.34 0.34 0.34 0.34 0.29 0.24 %  1168 /   887"""
import numpy as np
import pytest

import query_ex_util as qx
import query_util as qu
from vk_gltf_renderer_amd import pathtracer as ptmod

MODES = (("cutoff 0.5", dict(alpha=qx.CUTOFF, blend_threshold=0.5)), ("cutoff 0.9", dict(alpha=qx.CUTOFF, blend_threshold=0.9)),
         ("stochastic 1", dict(alpha=qx.STOCHASTIC, seed=1)), ("stochastic 99", dict(alpha=qx.STOCHASTIC, seed=99)),
         ("cull", dict(cull=qx.CULL_MATERIAL)), ("cutoff + cull", dict(alpha=qx.CUTOFF, cull=qx.CULL_MATERIAL)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return qx.Shim(tmp_path_factory.mktemp("host_shim_query_ex_ref"))


@pytest.mark.parametrize("name", qx.SCENES)
def test_reference_shares_outcomes_and_the_devices_per_ray_code(shim, tmp_path, name):
    scene = ptmod.Scene(qx.make_scene(name, tmp_path))
    st = qu.SceneTris(scene)
    sa = qx.SceneAlpha(scene, st)
    assert len(st) == scene.num_triangles > 0 and sa.tested.any()
    rays = qx.make_rays_ex(st, sa)
    assert len(rays) == 2048
    pairs = qu.Pairs(st, rays)
    # OPAQUE / NONE is query_util's reference, ray by ray
    plain, old = qx.ReferenceEx(pairs, qx.Decisions(pairs, sa)), qu.Reference(pairs)
    assert (plain.tri == old.tri).all() and (plain.ambiguous == old.ambiguous).all() and not plain.alpha_only.any()
    if name in qx.MEASURED:
        err_t, err_b = qu.measure_float32_error(st, rays, plain)
        print("QUERYREF_EX", name, "float32 against float64: t %.4e barycentrics %.4e" % (err_t, err_b), "recorded", qx.MEASURED[name])
        assert qx.MEASURED[name][0] * 0.999 <= err_t <= qx.MEASURED[name][0] * 1.001
        assert qx.MEASURED[name][1] * 0.999 <= err_b <= qx.MEASURED[name][1] * 1.001
    recs = qx.shim_records(st, sa)
    for label, kw in MODES:
        ref = qx.ReferenceEx(pairs, qx.Decisions(pairs, sa, **kw))
        share, alpha_only = float(ref.ambiguous.mean()), float(ref.alpha_only.mean())
        rejected, accepted = ref.outcome_shares()
        print("QUERYREF_EX", name, label, "ambiguous %.2f %% (alpha only %.2f %%)" % (100 * share, 100 * alpha_only), "rays with a rejected candidate",
              round(rejected * len(rays)), "with an accepted one", round(accepted * len(rays)), "hits", int(ref.hit.sum()))
        assert share <= qx.MAX_AMBIGUOUS_SHARE, (name, label, share)
        if label == "cutoff 0.5":
            assert rejected >= qx.MIN_OUTCOME_SHARE and accepted >= qx.MIN_OUTCOME_SHARE, (name, rejected, accepted)
        hits = shim.brute(*recs, rays, qx.rules(**kw))[:, 0]
        qu.check_hits(st, rays, ref, hits, *qx.TOLERANCE[name], what=name + ", " + label + " (host shim)")
    kw = dict(alpha=qx.CUTOFF, cull=qx.CULL_MATERIAL)
    ref = qx.ReferenceEx(pairs, qx.Decisions(pairs, sa, **kw))
    closest = shim.brute(*recs, rays, qx.rules(**kw))
    for k in (1, 3, 8):
        lists = shim.brute(*recs, rays, qx.rules(max_hits=k, **kw))
        qx.check_lists(st, rays, ref, lists, k, qx.TOLERANCE[name][0], what=name + " (host shim)")
        assert lists[:, :1].tobytes() == closest.tobytes()  # the first of the K nearest is the closest hit, bit for bit
    scene.close()
