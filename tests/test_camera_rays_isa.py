"""The compiled camera-ray kernels (csrc/device/camera_rays.hip; CPU-only: hipcc cross-compiles gfx950, tools/isa_census.py): the two streaming
kernels exist, go through global (not flat) loads and stores, keep everything in registers -- no scratch, no spills, no LDS, no full drain -- and
read their arguments through the scalar cache.  (k_selection_rays is a walk: it has the LDS stack of every per-lane walk and is not held to this.)"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402

KERNELS = ("k_generate_rays", "k_export_camera_rays")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("no hipcc")
    table = isa_census.census(source="camera_rays.hip")
    out = {}
    for name in KERNELS:
        hits = [v for k, v in table.items() if k.startswith("pt::" + name) or k.startswith(name)]
        assert len(hits) == 1, (name, sorted(table))
        out[name] = hits[0]
    assert sum(1 for k in table if "k_selection_rays" in k) == 2, sorted(table)  # both trees
    return out


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_has_no_scratch_spills_lds_or_generic_accesses(kernels, name):
    k = kernels[name]
    assert k["scratch"] == 0 and k["scratch_bytes"] == 0, k
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["flat_load"] == 0 and k["flat_store"] == 0, k
    assert k["drain"] == 0, k
    assert k["lds"] == 0, k


@pytest.mark.parametrize("name", KERNELS)
def test_arguments_arrive_through_the_scalar_cache(kernels, name):
    k = kernels[name]
    assert k["s_load"] >= 4 and k["sgpr_base_load"] == 0, k
    assert k["vgpr"] <= 64, k  # 256 threads of a streaming kernel: nowhere near a register budget that would cost occupancy


def test_memory_traffic_per_path(kernels):
    # generate: the two 16-byte words of the ray (+ the stored seed of a later sample).  export: the origin and direction records of queue 0 in, the two
    # words of the ray out
    g, e = kernels["k_generate_rays"], kernels["k_export_camera_rays"]
    assert 2 <= g["global_load"] <= 4 and g["global_store"] >= 4, g
    assert 2 <= e["global_load"] <= 3 and e["global_store"] == 2, e
