"""k_atrous, k_svgf_prepare, k_svgf_atrous and k_svgf_finish (csrc/device/denoise.hip) on the synthetic images of tests/image_pass_cases.py, case
by case against the float64 restatements of tests/denoise_ref.py.  tests/test_image_pass_reference.py proves those restatements and the cases on
the CPU.  One child process (tests/image_pass_device_child.py) runs every case; this module compares.

Tolerances are derived, not fitted (tests/denoise_ref.py has the counts, image_pass_cases.expected puts them together):
  structural   every weight is exactly 0 or 1, pixel values are small integers: one iteration costs at most STRUCT_C = 64 float32 roundings (25
               products counted once, 25 + 25 running additions, one division, 12 for three weight products and exp / pow landing next to 1),
               errors pass through later iterations convexly: iterations * 64 * 2^-24 * max|input| -- 3.8e-6 per iteration, where a wrong tap
               weight moves the result by about 1e-2.  Alpha is bit-exact.
  numerical    one edge-stopping term, one iteration: the result is a weight-normalised mean, so a weight error dw_i moves it by at most
               sum(dw_i |q_i - out|) / sum(w_i); dw_i per tap from the roundings of the argument and 2 ulp for __expf (one product by log2 e and
               the hardware exp2), expf and powf (the library's; __powf is __ocml_pow_f32 in __clang_hip_math.h), plus the structural term.
  joint        all terms on, several iterations: weight errors feed back through the colour / luminance terms, so the conditioning is MEASURED on
               the CPU, against the reference only (float32 restatement in the kernel's operation order against the float64 one); the device gets
               16 times that (1-2 ulp hardware transcendentals against numpy's half ulp, fused multiply-adds regrouping the sums, a sample
               maximum standing in for a worst case) plus the first iteration's numerical bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

import image_pass_cases as ipc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def device_results(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("image_passes") / "results.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "image_pass_device_child.py"), out], capture_output=True, text=True, timeout=180)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "IMAGE_PASS_DEVICE_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", ipc.all_cases(), ids=lambda c: c.name)
def test_device_matches_the_restatement(device_results, case):
    got = device_results[case.name]
    want, bound, disc = ipc.expected(case)
    assert got.shape == want.shape and np.isfinite(got).all()
    # alpha comes back bit for bit
    assert np.array_equal(got[..., 3].view(np.uint32), case.color[..., 3].view(np.uint32)), case.name
    if case.kind == "temporal":
        # an empty history: the spatial restatement wherever the first-hit id is valid (the box was rendered first, so motion exists)
        ids = device_results[case.name + "/first_hit"][..., 3].view(np.uint32)
        valid = ids != np.uint32(0xFFFFFFFF)
        assert valid.mean() > 0.5
        got = np.where(valid[..., None], got, want.astype(np.float32))
    ratio, err, b, (x, y, ch), border = ipc.worst(got, want, bound)
    print(f"IMAGE_PASS_ROW | {case.name} | {disc:.3e} | {b:.3e} | {err:.3e} | {ratio:.3f} |")
    assert ratio <= 1.0, (f"{case.name}: worst pixel x={x} y={y} channel={ch}, {border} from the border: got {got[y, x, ch]!r}, want {want[y, x, ch]!r}, "
                          f"error {err:.3e} > bound {b:.3e}")
