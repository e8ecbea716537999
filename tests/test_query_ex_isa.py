"""The compiled kernels of the _ex ray queries (csrc/device/query.hip; CPU-only: hipcc cross-compiles gfx950, tools/isa_census.py): they exist,
use no flat loads or stores, spill no vector register, and need no more scratch than the plain closest-hit kernel of the same tree -- which
already carries the private overflow stack: the list of the K nearest hits lives in registers and adds none.  The six kernels of the plain entry
points are what profiles/query_ex_census.txt records (identical before and after the _ex kernels were added)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402

EX = [("true" if wide else "false", "true" if any_ else "false", k) for wide in (True, False) for any_, k in ((True, 1), (False, 1), (False, 2), (False, 4), (False, 8))]
PLAIN = ("k_query_rays<true, true>", "k_query_rays<true, false>", "k_query_rays<false, true>", "k_query_rays<false, false>", "k_pick_rays<true>",
         "k_pick_rays<false>")


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("no hipcc")
    return isa_census.census(source="query.hip")


@pytest.mark.parametrize("wide,any_,k", EX)
def test_ex_kernel_uses_global_memory_spills_nothing_and_adds_no_scratch(table, wide, any_, k):
    name = "k_query_rays_ex<%s, %s, %d>" % (wide, any_, k)
    assert name in table, sorted(table)
    kern, plain = table[name], table["k_query_rays<%s, false>" % wide]
    assert kern["flat_load"] == 0 and kern["flat_store"] == 0, kern
    assert kern["vgpr_spill"] == 0, kern
    assert kern["scratch_bytes"] <= plain["scratch_bytes"], (kern, plain)
    assert kern["global_store"] == 4 * k, kern  # K records of four 16-byte stores
    assert kern["vgpr"] <= 256, kern            # two blocks of 256 lanes per CU


def test_pick_ray_kernel_and_the_plain_kernels_as_recorded(table):
    k = table["k_pick_make_rays"]
    assert k["scratch_bytes"] == 0 and k["flat_load"] == 0 and k["flat_store"] == 0 and k["vgpr_spill"] == 0 and k["global_store"] == 2, k
    text = open(os.path.join(ROOT, "profiles", "query_ex_census.txt")).read()
    for name in PLAIN:
        m = re.search(r"^after +%s +(.*)$" % re.escape(name), text, re.M)
        assert m, name
        assert [int(x) for x in m.group(1).split()] == [table[name][key] for key in isa_census.KEYS], (name, table[name])
