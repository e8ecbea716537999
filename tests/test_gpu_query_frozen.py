"""Frozen digests of the ray queries (csrc/device/query.hip, pt_lane_walk.h, pt_query.h) and of the selection image (k_selection): SHA-256 over
the returned records of the mixed alpha + glass scene of tests/query_ex_util.py at 128 x 96, on the 8-wide tree and on the BVH2, with the rays of
query_ex_util.make_rays_ex -- CLOSEST, NEAREST_K 4 under plain rules, CUTOFF 0.5 + CULL_MATERIAL, STOCHASTIC seed 9, NEAREST_K 8 under CUTOFF, pick
at every pixel centre (plain, and alpha="cutoff", cull="material"), read_selection() after a first frame, and batches of 1, 65 and 257 rays (one
lane, the first lane of a second wave, the first lane of a second block).

The expected digests (tests/golden/query_frozen.json) were recorded from the commit BEFORE the query calls shared one walk and one host path, on
an MI355X: a change to the query subsystem that is meant to return the same records is checked against what the code returned before it, not
against itself.  To record: run this file with MI_PT_WRITE_QUERY_DIGESTS naming the file to write; it then writes and compares nothing.

ANY returns the first accepted triangle the walk meets, which depends on the tree the builder made.  When the file was recorded, two fresh
instances per tree returned equal ANY bytes (the file's "any_records" entry says "full"), so ANY's full records are digested, under plain rules
and under CUTOFF + CULL_MATERIAL.  Were it "hit_bit", only the MI_PT_HIT bit of each record would be."""
import hashlib
import json
import os

import numpy as np
import pytest

import parity_util as pu
import query_ex_util as qx
import query_util as qu
from test_gpu_refit import _render, _tracer
from vk_gltf_renderer_amd import _capi as capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "query_frozen.json")
WRITE = os.environ.get("MI_PT_WRITE_QUERY_DIGESTS")
W, H = 128, 96
TREES = {"8-wide": 0, "BVH2": 1}
ANY_RULES = (("any", dict(mode="any")), ("any cutoff material", dict(mode="any", alpha="cutoff", cull="material")))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _any_digest(hits, full):
    return _sha(hits) if full else _sha((hits["flags"] & capi.MI_PT_HIT).astype(np.uint8))


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """{tree: {what: digest}} of the library under test, and whether ANY is digested in full (decided when recording, read from the file otherwise)."""
    st = pu.Setup(qx.make_scene("mixed_alpha_glass", tmp_path_factory.mktemp("gpu_query_frozen")), W, H, max_depth=2)
    tris = qu.SceneTris(st.scene)
    rows = qu.as_rows(qx.make_rays_ex(tris, qx.SceneAlpha(st.scene, tris)))
    ys, xs = np.mgrid[0:H, 0:W]
    centres = np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], 1).astype(np.float32)
    full = True
    if WRITE:
        for bvh in TREES.values():
            a, b = _tracer(st, bvh=bvh), _tracer(st, bvh=bvh)
            full = full and all(a.query_rays(rows, **kw).tobytes() == b.query_rays(rows, **kw).tobytes() for _, kw in ANY_RULES)
            a.close()
            b.close()
    else:
        full = json.load(open(GOLDEN))["any_records"] == "full"
    out = {}
    for tree, bvh in TREES.items():
        tr = _tracer(st, bvh=bvh)
        d = out[tree] = {}
        d["closest"] = _sha(tr.query_rays(rows))
        d["nearest_k 4"] = _sha(tr.query_rays(rows, mode="nearest_k", max_hits=4))
        d["cutoff 0.5 material"] = _sha(tr.query_rays(rows, alpha="cutoff", blend_threshold=0.5, cull="material"))
        d["stochastic seed 9"] = _sha(tr.query_rays(rows, alpha="stochastic", seed=9))
        d["nearest_k 8 cutoff"] = _sha(tr.query_rays(rows, mode="nearest_k", max_hits=8, alpha="cutoff"))
        for what, kw in ANY_RULES:
            d[what] = _any_digest(tr.query_rays(rows, **kw), full)
        for n in (1, 65, 257):
            d["closest, %d rays" % n] = _sha(tr.query_rays(rows[-n:]))
            d["nearest_k 4 cutoff material, %d rays" % n] = _sha(tr.query_rays(rows[-n:], mode="nearest_k", max_hits=4, alpha="cutoff", cull="material"))
        d["pick"] = _sha(tr.pick(centres))
        d["pick cutoff material"] = _sha(tr.pick(centres, alpha="cutoff", cull="material"))
        _render(tr, st, frames=1)
        sel = tr.read_selection()
        assert 0.05 < (sel > 0).mean() < 1.0  # the camera sees the scene and some background
        d["selection"] = _sha(sel)
        tr.close()
    st.scene.close()
    if WRITE:
        with open(WRITE, "w") as f:
            json.dump({"any_records": "full" if full else "hit_bit", "digests": out}, f, indent=1, sort_keys=True)
            f.write("\n")
    return out


@pytest.mark.parametrize("tree", sorted(TREES))
def test_records_are_the_frozen_ones(recorded, tree):
    if WRITE:
        return
    expected = json.load(open(GOLDEN))["digests"][tree]
    assert sorted(recorded[tree]) == sorted(expected)
    for what, digest in recorded[tree].items():
        print("QUERY_FROZEN", tree, what, digest, "ok" if digest == expected[what] else "DIFFERS from " + expected[what])
    assert not [what for what, digest in recorded[tree].items() if digest != expected[what]]
