"""The any-hit shadow walk adds an unoccluded ray's term with three float atomics nobody waits for -- in the COMPILED code (LABNOTES.md, "The shadow
walk deposits its own results").  The images do not change whichever way the sum is formed, so no parity test notices the deposit turning back into
a load / add / store, a compare-and-swap loop or an atomic that returns its value (and makes the wave wait for it) -- the generated code does.

Checked on k_trace_shadow<true, 0, false> and <true, 1, false>, the two 8-wide instantiations the benchmark workloads run:
  * the source lines of shadowDepositAdd (pt_scene.h) map to exactly three global_atomic_add_f32, none of them with a returned value (no `sc0`, no
    destination register), and the kernel has no other float atomic: the deposit has one place in the kernel;
  * no global_atomic_cmpswap anywhere in either kernel;
  * nothing spilled in <true, 1, false>, which sits at its 128 VGPRs (tests/test_isa_census.py allows the walks a few spills of the ray feed; the
    state the deposit keeps alive must not add any -- it did until the contribution was asked for again when the ray starts);
  * <true, 1, false> asks for the contribution when the ray starts: three single-word loads in one block with no vector-memory wait behind them there;
  * control: the recording walk <true, 3, false>, which hands every ray to k_shadow_resolve, has no float atomic at all -- what the same condition
    finds in the walks of a tree without the deposit.
The places are found through the line table (-gline-tables-only), as in tests/test_walk_overlap_isa.py.  CPU-only: hipcc cross-compiles gfx950 without
a GPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402  (HIPCC, DEVICE)

KERNELS = {"<true, 0, false>": "k_trace_shadowILb1ELi0ELb0E", "<true, 1, false>": "k_trace_shadowILb1ELi1ELb0E"}
CONTROL = {"<true, 3, false>": "k_trace_shadowILb1ELi3ELb0E"}


def _command(out):
    return [isa_census.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "-I" + isa_census.DEVICE,
            "-Wno-unused-function", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-freciprocal-math", "-fapprox-func",  # (csrc/Makefile: PT_KERNELS_FP)
            "--cuda-device-only", "-S", "-gline-tables-only", "-o", out, os.path.join(isa_census.DEVICE, "pt_kernels.hip")]


def _deposit_lines():
    """1-based numbers of the lines of shadowDepositAdd's body (pt_scene.h) that hold an atomic add."""
    lines = open(os.path.join(isa_census.DEVICE, "pt_scene.h")).read().split("\n")
    start = next(i for i, l in enumerate(lines) if "void shadowDepositAdd(" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("}"))
    hits = [i + 1 for i in range(start, end) if "__hip_atomic_fetch_add(" in lines[i]]
    assert len(hits) == 3, hits
    return hits


def _kernel(text, mangled):
    """The instructions of one kernel in layout order: (mnemonic and operands, (file, line) of the line table or None, number of its basic block)."""
    files, out, inside, loc, block = {}, [], False, None, 0
    for line in text.split("\n"):
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"\s+"([^"]*)"', line)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3))
            continue
        m = re.match(r"^(_Z\w+):", line)
        if m:
            inside = mangled in m.group(1)
            continue
        if not inside:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            inside = False
            continue
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            loc = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        if re.match(r"^\.LBB\w+:", line) or re.match(r"^; %bb\.\d+:", line):
            block += 1
            continue
        t = line.strip()
        if re.match(r"^[a-z]\w*", t):
            out.append((re.sub(r"\s*;.*$", "", t), loc, block))
    assert out, mangled
    return out


def _spills(text, mangled):
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name and mangled in name.group(1):
            return int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
    raise AssertionError(mangled)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("shadow_deposit_isa") / "lines.s")
    r = subprocess.run(_command(out), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def deposit_atomics(kernel, lines):
    """(the deposit's float atomics, every other float atomic of the kernel)"""
    at = [e for e in kernel if e[0].startswith(("global_atomic_add_f32", "flat_atomic_add_f32", "global_atomic_pk_add", "buffer_atomic_add_f32"))]
    mine = [e for e in at if e[1] is not None and e[1][0] == "pt_scene.h" and e[1][1] in lines]
    return mine, [e for e in at if e not in mine]


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_the_deposit_is_three_float_atomics_without_a_returned_value(compiled, name):
    k = _kernel(compiled, KERNELS[name])
    lines = _deposit_lines()
    mine, others = deposit_atomics(k, lines)
    print(name, [e[0] for e in mine])
    assert len(mine) == 3 and not others, (mine, others)
    assert sorted(e[1][1] for e in mine) == lines  # one instruction per source line
    for ins, _, _ in mine:
        # no-return form: address pair, data, `off` (or an SGPR base) -- a returning one has a destination register in front and carries sc0
        assert re.match(r"^global_atomic_add_f32 v\[\d+:\d+\], v\d+, (off|s\[\d+:\d+\])( offset:\d+)?$", ins), ins


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_no_compare_and_swap_loop(compiled, name):
    assert not [e[0] for e in _kernel(compiled, KERNELS[name]) if "atomic_cmpswap" in e[0]]


def test_the_deposit_spills_nothing_in_the_alpha_tested_walk(compiled):
    vgpr, spilled = _spills(compiled, KERNELS["<true, 1, false>"])
    assert vgpr <= 128 and spilled == 0, (vgpr, spilled)


def _late_load_lines():
    """1-based numbers of the three lines of k_trace_shadow (pt_kernels.hip) that ask for the contribution when the ray starts."""
    lines = open(os.path.join(isa_census.DEVICE, "pt_kernels.hip")).read().split("\n")
    hits = [i + 1 for i, l in enumerate(lines) if re.search(r"contrib\.[xyz] = __hip_atomic_load\(", l)]
    assert len(hits) == 3, hits
    return hits


def test_the_late_contribution_load_is_three_words_nobody_waits_for(compiled):
    """<true, 1, false> asks for the contribution when the ray starts (LATE_CONTRIB).  Its shape is tuned against the compiler -- a three-word load wants
    consecutive registers and the copies out of them brought `s_waitcnt vmcnt(0)` right behind it; inside the ray-start block the loads landed in front of
    that block's wait for the prefetched words -- so the shape is pinned: three single-word loads, one per source line, in one basic block, and no
    vector-memory wait behind them in that block."""
    k = _kernel(compiled, KERNELS["<true, 1, false>"])
    lines = _late_load_lines()
    at = [i for i, e in enumerate(k) if e[0].startswith("global_load") and e[1] is not None and e[1][0] == "pt_kernels.hip" and e[1][1] in lines]
    print([k[i] for i in at])
    assert len(at) == 3 and sorted(k[i][1][1] for i in at) == lines, [k[i] for i in at]
    assert all(re.match(r"^global_load_dword v\d+,", k[i][0]) for i in at), [k[i][0] for i in at]
    assert len({k[i][2] for i in at}) == 1
    behind = [k[i][0] for i in range(at[0], len(k)) if k[i][2] == k[at[0]][2] and k[i][0].startswith("s_waitcnt") and "vmcnt" in k[i][0]]
    assert not behind, behind
    # ... and the instantiation with registers to spare keeps the contribution of the prefetch: no such load
    k0 = _kernel(compiled, KERNELS["<true, 0, false>"])
    assert not [e for e in k0 if e[0].startswith("global_load") and e[1] is not None and e[1][0] == "pt_kernels.hip" and e[1][1] in lines]


def test_a_walk_without_the_deposit_fails_the_condition(compiled):
    """The issue asks that the PARENT's assembly fail the first condition.  A test cannot compile another commit; the recording walk of this tree, which
    deposits nothing in the walk, stands in for it (the parent's own <true, 0, false> and <true, 1, false> were compiled by hand for LABNOTES: no float
    atomic in either)."""
    mine, others = deposit_atomics(_kernel(compiled, CONTROL["<true, 3, false>"]), _deposit_lines())
    assert not mine and not others
