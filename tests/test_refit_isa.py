"""The compiled refit kernels (csrc/device/bvh_refit.hip; CPU-only: hipcc cross-compiles gfx950, tools/isa_census.py): they exist, read and
write through global (not flat) loads and stores, and spill nothing."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402

KERNELS = ("k_refit_tris", "k_refit_level", "k_sah_partial", "k_sah_final")


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("no hipcc")
    return isa_census.census(source="bvh_refit.hip")


@pytest.mark.parametrize("name", KERNELS)
def test_refit_kernel_uses_global_memory_and_spills_nothing(table, name):
    hits = [v for k, v in table.items() if k.split("::")[-1] == name or k == name]
    assert len(hits) == 1, sorted(table)
    k = hits[0]
    assert k["scratch"] == 0 and k["scratch_bytes"] == 0, k
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["flat_load"] == 0 and k["flat_store"] == 0, k
    assert k["global_load"] >= 1 and k["global_store"] >= 1, k


def test_level_kernel_fits_the_register_file_of_two_waves(table):
    k = [v for n, v in table.items() if n.endswith("k_refit_level")][0]
    assert k["vgpr"] <= 256, k
