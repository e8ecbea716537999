"""Every entry point of libmi_pt.so that takes the instance refuses (or accepts) a NULL instance before it touches HIP: the return value and
the mi_pt_last_error() text of each such call, against tests/golden/api_null_refusals.json.  Runs without a GPU.

The golden file is written by this module run as a script (`python tests/test_api_refusals.py --write`) and changes only together with the
messages or the entry points themselves."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vk_gltf_renderer_amd import _capi as capi  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "api_null_refusals.json")

# Entry points left out because the call does not return cleanly: none.  (An entry may be added only with the reason next to it.)
LEFT_OUT = {}

# The message every call starts from: mi_pt_last_error() keeps the last refusal, so a call that succeeds (mi_pt_destroy(NULL)) would otherwise
# report whatever ran before it.
PRIME = "mi_pt_synchronize"


def _zero(argtype):
    """NULL for pointers, 0 for numbers."""
    if issubclass(argtype, (C._Pointer, C.c_void_p, C.c_char_p)):
        return None
    return argtype(0)


def instance_entry_points():
    return sorted(n for n, (_, args) in capi.PT_SYMBOLS.items() if args and args[0] is C.c_void_p and n not in LEFT_OUT)


def null_refusals():
    lib = capi.pt_lib()
    out = {}
    for name in instance_entry_points():
        res, args = capi.PT_SYMBOLS[name]
        assert lib.mi_pt_synchronize(None) != 0
        rc = getattr(lib, name)(*[_zero(a) for a in args])
        out[name] = [rc if res is not C.c_void_p else (rc or 0), lib.mi_pt_last_error().decode()]
    return out


def test_null_instance_refusals_match_the_recorded_ones():
    if not os.path.exists(os.path.join(capi.LIB_DIR, "libmi_pt.so")):
        pytest.skip("libmi_pt.so not built yet (run __graft_entry__.build())")
    want = json.load(open(GOLDEN))
    got = null_refusals()
    assert sorted(got) == sorted(want)  # every instance entry point of the binding, and no other
    assert not LEFT_OUT
    assert {n: v for n, v in got.items() if v != want[n]} == {}


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_api_refusals.py --write")
    with open(GOLDEN, "w") as f:
        json.dump(null_refusals(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
