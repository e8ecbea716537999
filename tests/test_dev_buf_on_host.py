"""pt::DevBuf, the owner of every device allocation (csrc/device/dev_buf.h), on the host: a stand-alone program over the counting
hipMalloc / hipFree / hipMemcpy stand-ins of tests/host_shim, built with the address and undefined-behaviour sanitizers and run as a
child process.  It exits non-zero on any mismatch; the sanitizer turns a double free or a leak into a failure."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_buf_moves_frees_once_and_survives_failed_allocations(tmp_path):
    exe = str(tmp_path / "dev_buf_on_host")
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",  # (the runtimes linked in: nothing to preload, and no library-order check at start)
                    "-I" + shim, "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"), os.path.join(shim, "dev_buf_on_host.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed expectations" in r.stdout, r.stdout
