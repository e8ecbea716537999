"""CPU tier of the device known-answer tests (tests/test_gpu_device_kat.py): the test-only library tests/device_kat/libmi_pt_kat.so exists
after build(), exports every launcher the GPU test binds, and its object is compiled with exactly the floating-point flags of pt_kernels.o --
otherwise the GPU test would be looking at arithmetic the product does not ship."""
import os
import re
import subprocess

import device_kat_lib as kat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc")
FP_FLAG = re.compile(r"^-f(no-)?(hip-fp32|reciprocal-math|approx-func|fast-math|finite-math|unsafe-math|associative-math|signed-zeros|denormal|fp-contract|fp-model|gpu-flush)"
                     r"|^-m(no-)?(daz|unsafe-fp)|^-O|^-DPT_|^-DMI_PT_EXACT_FP")


def _compile_lines():
    """`make -n -B`: every command a from-scratch build would run, keyed by the object it writes."""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC], check=True, capture_output=True, text=True).stdout
    lines = {}
    for line in out.splitlines():
        m = re.search(r" -c -o (\S+\.o) ", line)
        if m:
            lines[os.path.basename(m.group(1))] = line.split()
    return lines


def test_library_is_built_and_exports_every_launcher():
    assert os.path.exists(kat.PATH), "tests/device_kat/libmi_pt_kat.so is missing: __graft_entry__.build() builds it (csrc/Makefile, part of `all`)"
    nm = subprocess.run(["nm", "-D", "--defined-only", kat.PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    missing = sorted(set(kat.LAUNCHERS) - exported)
    assert not missing, missing
    # the product library gains nothing from the test library
    pt = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vk_gltf_renderer_amd", "lib", "libmi_pt.so")], check=True, capture_output=True, text=True).stdout
    assert "kat_" not in pt
    ldd = subprocess.run(["ldd", kat.PATH], capture_output=True, text=True).stdout
    assert "libmi_pt.so" not in ldd and "libmi_host.so" not in ldd, ldd


def test_kat_object_is_compiled_with_the_floating_point_flags_of_pt_kernels():
    lines = _compile_lines()
    assert {"pt_kernels.o", "kat_device.o", "kat_device_ieee.o", "mi_pt_api.o"} <= set(lines), sorted(lines)
    fp = lambda obj: sorted(t for t in lines[obj] if FP_FLAG.search(t))
    arch = lambda obj: sorted(t for t in lines[obj] if t.startswith("--offload-arch"))
    assert fp("kat_device.o") == fp("pt_kernels.o"), (fp("kat_device.o"), fp("pt_kernels.o"))
    assert {"-fno-hip-fp32-correctly-rounded-divide-sqrt", "-freciprocal-math", "-fapprox-func"} <= set(fp("kat_device.o"))
    # ... everything else too, apart from the source, the object and nothing more
    strip = lambda obj: sorted(t for t in lines[obj] if not t.endswith((".hip", ".o")))
    assert strip("kat_device.o") == strip("pt_kernels.o"), (strip("kat_device.o"), strip("pt_kernels.o"))
    # the IEEE object of the exact-math group: the flags of every other device object (no fast option), plus its -DKAT_IEEE
    assert fp("kat_device_ieee.o") == fp("mi_pt_api.o")
    assert [t for t in strip("kat_device_ieee.o") if t not in strip("mi_pt_api.o")] == ["-DKAT_IEEE"]
    assert arch("kat_device.o") == arch("kat_device_ieee.o") == ["--offload-arch=gfx950"]
    # the source defines PT_FAST_SHADING_MATH for the fast object exactly as pt_kernels.hip does
    src = open(os.path.join(ROOT, "tests", "device_kat", "kat_device.hip")).read()
    assert re.search(r"#ifndef KAT_IEEE\s*\n#define PT_FAST_SHADING_MATH 1", src)
