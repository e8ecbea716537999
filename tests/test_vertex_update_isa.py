"""The compiled vertex-update kernels (csrc/device/vertex_update.hip; CPU-only: hipcc cross-compiles gfx950, tools/isa_census.py): both exist,
stream through global (not flat) loads and stores, keep everything in registers -- no scratch, no spills, no LDS -- and read their
block-uniform task record through the scalar cache."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402

KERNELS = ("k_vertex_ingest", "k_rebuild_normals")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("no hipcc")
    table = isa_census.census(source="vertex_update.hip")
    out = {}
    for name in KERNELS:
        hits = [v for k, v in table.items() if k.startswith("pt::" + name) or k.startswith(name)]
        assert len(hits) == 1, (name, sorted(table))
        out[name] = hits[0]
    return out


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_has_no_scratch_spills_lds_or_generic_accesses(kernels, name):
    k = kernels[name]
    assert k["scratch"] == 0 and k["scratch_bytes"] == 0, k
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["flat_load"] == 0 and k["flat_store"] == 0, k
    assert k["drain"] == 0, k
    assert k["lds"] == 0, k


def test_task_records_arrive_through_the_scalar_cache(kernels):
    # the kernel arguments, the block -> task entry and the record (7 pointers + 4 words; 6 pointers + 4 words) are s_load, not per-lane loads
    for name in KERNELS:
        assert kernels[name]["s_load"] >= 4 and kernels[name]["sgpr_base_load"] == 0, (name, kernels[name])
    # ingest: one load per supplied stream (positions, normals, tangents), nothing read back from the resident record; stores to the three
    # streams and the record.  rebuild: the run ends, a corner, its triangle's indices and three positions; the stream and the record.
    assert kernels["k_vertex_ingest"]["global_load"] == 3 and kernels["k_vertex_ingest"]["global_store"] >= 5, kernels["k_vertex_ingest"]
    assert kernels["k_rebuild_normals"]["global_load"] >= 6 and kernels["k_rebuild_normals"]["global_store"] >= 2, kernels["k_rebuild_normals"]
    # 256 threads of a copy kernel: nowhere near a register budget that would cost occupancy
    for name in KERNELS:
        assert kernels[name]["vgpr"] <= 64, (name, kernels[name])
