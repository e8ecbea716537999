"""The compiled deformation kernel (csrc/device/deform.hip; CPU-only: hipcc cross-compiles gfx950, tools/isa_census.py): it exists, streams
through global (not flat) loads and stores with counted waits, keeps everything in registers, and reads its block-uniform task record and
the morph weights through the scalar cache."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402


@pytest.fixture(scope="module")
def kernel():
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("no hipcc")
    table = isa_census.census(source="deform.hip")
    hits = [v for k, v in table.items() if k.startswith("pt::k_deform") or k.startswith("k_deform")]
    assert len(hits) == 1, sorted(table)
    return hits[0]


def test_deform_kernel_has_no_scratch_spills_or_generic_accesses(kernel):
    assert kernel["scratch"] == 0 and kernel["scratch_bytes"] == 0, kernel
    assert kernel["vgpr_spill"] == 0 and kernel["sgpr_spill"] == 0, kernel
    assert kernel["flat_load"] == 0 and kernel["flat_store"] == 0, kernel
    assert kernel["drain"] == 0, kernel
    assert kernel["lds"] == 0, kernel  # (the joint tables are read from L1 / L2: LABNOTES.md)


def test_deform_kernel_reads_its_task_record_through_the_scalar_cache(kernel):
    # the task record (13 pointers + 8 words) and the block -> task entry arrive as s_load, not as per-lane vector loads
    assert kernel["s_load"] >= 5, kernel
    assert kernel["global_load"] >= 8 and kernel["global_store"] >= 4, kernel
