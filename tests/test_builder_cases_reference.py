"""The yardstick of tests/test_gpu_builder_matrix.py, checked without a GPU: on every case of tests/builder_cases.py the float64 reference marks
at most 1 % of the case's rays ambiguous and at least 30 % of them hit; the float32 ray / triangle test differs from float64 by no more than
builder_cases.MEASURED records (the GPU tolerance is 8 x that); and the properties a case exists for hold in float32 restatements of the builder's
stages: one Morton key for the whole cluster of `one_cell`, zero centroid extents in `line` and the flat sheets, exact vertices in `offset`, and
a PLOC tree as deep as its leaves are many for the chains (deeper than the BVH2 walk's stack, pt_bvh.h)."""
import numpy as np
import pytest

import builder_cases as bc
import query_util as qu
from vk_gltf_renderer_amd import pathtracer as ptmod


def test_every_case_is_recorded():
    assert set(bc.MEASURED) == set(bc.NAMES)


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_reference(tmp_path, name):
    scene = ptmod.Scene(bc.make_scene(name, tmp_path))
    whole = qu.SceneTris(scene)
    st = qu.SceneTris(scene, nodes=bc.reference_nodes(name))
    assert 0 < len(whole) == scene.num_triangles <= 2100
    rays = bc.make_rays(name, st)
    assert len(rays) == bc.NUM_RAYS and rays.dtype == qu.RAY_DTYPE
    assert np.isfinite(rays["origin"]).all() and (np.abs(np.linalg.norm(rays["direction"].astype(np.float64), axis=1) - 1.0) < 1e-6).all()
    ref = qu.Reference(qu.Pairs(st, rays))
    share = float(ref.ambiguous.mean())
    print("BUILDERCASE", name, "triangles", len(whole), "hits", int(ref.hit.sum()), "ambiguous share %.4f %%" % (100 * share))
    assert share <= qu.MAX_AMBIGUOUS_SHARE
    assert ref.hit.sum() >= 0.3 * len(rays)
    err_t, err_b = qu.measure_float32_error(st, rays, ref)
    print("BUILDERCASE", name, "float32 against float64: t %.4e barycentrics %.4e" % (err_t, err_b), "recorded", bc.MEASURED.get(name))
    assert err_t <= bc.MEASURED[name][0] * 1.001 and err_b <= bc.MEASURED[name][1] * 1.001

    keys, q = bc.morton(whole.V32)
    if name.startswith("counts_"):
        assert len(whole) == int(name[7:])
    if name == "one_cell":
        cluster = np.abs(whole.V).max((1, 2)) < 4.0
        assert cluster.sum() == 500 and len(whole) == 502
        assert len(np.unique(keys[cluster])) == 1 and len(np.unique(keys)) == 3  # all 500 in one cell, the far two in the corner cells
        assert len(np.unique(whole.V[cluster].reshape(500, 9), axis=0)) == 500 and whole.V[cluster].min() >= 0.0 and whole.V[cluster].max() < 0.25
    if name == "copies":
        assert len(whole) == 40 * len(st) == 1280 and (whole.V.reshape(40, -1) == whole.V.reshape(40, -1)[0]).all()
        assert (whole.node == np.repeat(np.arange(40), 32)).all()
    if name.startswith("flat_"):
        axis = "xyz".index(name[5])
        assert (whole.V32[:, :, axis] == np.float32(3.3)).all() and (q[:, axis] == 0).all() and len(np.unique(q[:, (axis + 1) % 3])) > 100
    if name == "line":
        assert len(whole) == 300 and (q[:, 1] == 0).all() and (q[:, 2] == 0).all() and len(np.unique(q[:, 0])) == 300
    if name == "offset":
        assert (whole.V == whole.V32.astype(np.float64)).all() and whole.V.min() > 65530.0 and (whole.V * 64 == np.round(whole.V * 64)).all()
        assert np.abs(rays["origin"] - 0.5 * (whole.lo + whole.hi)).max() < 8.0 + 0.5 * (whole.hi - whole.lo).max()
    if name == "scales":
        assert len(whole) == 13 * 8
    if name == "needles":
        lo, hi = bc.boxes32(whole.V32[:64])
        assert (np.linalg.norm(hi - lo, axis=1) > 999.0).all() and ((hi - lo).min(1) > 150.0).all()  # diagonal: no thin box
    if name in bc.CHAINS:
        shells = bc.CHAINS[name][0]
        assert len(whole) == shells and (whole.node == np.arange(shells)).all()
        assert len(np.unique(ref.tri[ref.hit])) >= 40
        depth, rounds = bc.ploc_depth(whole.V32)
        print("BUILDERCASE", name, "PLOC restatement: depth", depth, "in", rounds, "rounds")
        assert depth >= shells - 1
    scene.close()
