"""Records what tests/test_gpu_builder_fingerprint.py compares, with the library MI_PT_LIB selects (default: the tree's own).
usage: python tools/record_builder_fingerprints.py OUT.json      (record twice and diff: a field that differs between two runs pins nothing)"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_builder_fingerprint as fp  # noqa: E402

with tempfile.TemporaryDirectory() as d:
    record = {name: fp.fingerprint(name, d) for name in fp.CASES}
with open(sys.argv[1], "w") as f:
    json.dump(record, f, indent=1, sort_keys=True)
    f.write("\n")
print("recorded", len(record), "cases x", len(fp.CONFIGS), "configurations")
