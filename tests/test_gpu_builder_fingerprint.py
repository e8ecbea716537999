"""What the acceleration-structure builder makes of the cases of tests/builder_cases.py, pinned field by field against
tests/golden/builder_fingerprints.json: a restructuring of buildBvh / buildBvh8 (csrc/device/bvh_build.hip, bvh8.hip) must build the tree it built
before.  Per case -- every name of builder_cases.NAMES (counts_2: fewer than three inner BVH2 nodes) and `one_triangle`, the scene without a BVH2
inner node that only the host collapse serves -- one instance per configuration A, B, C, E, F, I of tests/test_gpu_builder_matrix.py, and of each

  bvhNodeCount, bvhTriangleCount, bvhNodeBytes                     (mi_pt_get_stats)
  the six traversal counters and surfaceHits of one 40 x 24 frame at maxDepth 3 with collectCounters on
  the SHA-1 of that frame's accumulator
  for A, C, E, I after mi_pt_set_accel_update(REFIT), which builds again and keeps the refit data: sahCostAtBuild (the double's bits, as hex)
  and refitBytes.

The file was recorded twice with the library of the commit before the builder was cut into phases (tools/record_builder_fingerprints.py); the
two recordings agree in every field of every case and configuration, so nothing is dropped from the comparison: DROPPED is empty, and every
field is compared exactly."""
import hashlib
import json
import os

import numpy as np
import pytest

import builder_cases as bc
import parity_util as pu
from test_gpu_builder_matrix import CONFIGURATIONS
from test_gpu_query import _environment
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "builder_fingerprints.json")
CASES = bc.NAMES + ("one_triangle",)
CONFIGS = tuple(c for c in CONFIGURATIONS if c[0] in "ABCEFI")
REFIT_CONFIGS = "ACEI"
STATS = ("bvhNodeCount", "bvhTriangleCount", "bvhNodeBytes", "nodesClosest", "trisClosest", "nodesShadow", "trisShadow", "nodesPrimary", "trisPrimary",
         "surfaceHits")
DROPPED = ()  # (case, configuration, field) that differed between the two recordings: none did


def make_scene(name, directory):
    if name == "one_triangle":
        return bc._save(os.path.join(str(directory), name + ".glb"), [(np.array([[0.2, 0.1, 0.3], [0.9, 0.2, 0.4], [0.4, 0.8, 0.6]]), None, [{}])])
    return bc.make_scene(name, directory)


def fingerprint(name, directory):
    """{configuration: record} of case `name`."""
    s = pu.Setup(make_scene(name, directory), 40, 24, max_depth=3)
    out = {}
    for cfg, bvh, switches in CONFIGS:
        with _environment(switches):
            tr = ptmod.PathTracer(s.scene, bvh=bvh, collect_counters=True)
        try:
            tr.resize(s.width, s.height)
            tr.set_frame_info(s.frame_info)
            tr.set_sky(s.sky)
            tr.render_frame(s.frame_params(0, 0))
            accum = tr.read_accum()
            stats = tr.stats()
            rec = {k: stats[k] for k in STATS}
            rec["accumSha1"] = hashlib.sha1(accum.tobytes()).hexdigest()
            if cfg in REFIT_CONFIGS:
                with _environment(switches):  # (the build of the switch reads the same switches)
                    tr.set_accel_update(capi.MI_PT_ACCEL_REFIT)
                a = tr.accel_info()
                rec["sahCostAtBuild"] = float(a["sahCostAtBuild"]).hex()
                rec["refitBytes"] = int(a["refitBytes"])
        finally:
            tr.close()
        out[cfg] = rec
    s.scene.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fingerprint_covers_every_case(golden):
    assert set(golden) == set(CASES)
    for name in CASES:
        assert set(golden[name]) == {c[0] for c in CONFIGS}, name


@pytest.mark.parametrize("name", CASES)
def test_builder_fingerprint(tmp_path, golden, name):
    got = fingerprint(name, tmp_path)
    differing = []
    for cfg, rec in got.items():
        want = golden[name][cfg]
        assert set(rec) == set(want), (name, cfg)
        for field, value in rec.items():
            if value != want[field] and (name, cfg, field) not in DROPPED:
                differing.append((cfg, field, value, want[field]))
    assert not differing, differing
