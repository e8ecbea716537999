"""The closest-hit walk keeps the triangle records of a round in flight across its node step -- in the COMPILED code (LABNOTES.md, "The triangle
fetch overlaps the node step").  The source always said so (TriRound, pt_kernels.hip); until the round was restructured the generated code waited
for every triangle load right where it was issued, and every pop of the per-lane stack drained the vector-memory counter for the sake of an
overflow branch almost no lane takes.  No pixel changes either way, so no parity test notices this coming back -- the generated code does.

Checked on k_trace_closest<true, true, false> and <true, false, false>, the two 8-wide instantiations the benchmark runs:
  * wait condition: from the first triangle-record load of triRoundPublish to the first node-record load of the node step behind it, no s_waitcnt
    asks for a vmcnt below the number of triangle loads issued so far (vector-memory results return in order: such a wait stalls on a triangle
    record).  One wait is exempt: the one LaneStack2::pop places behind its own scratch loads, inside the overflow branch (stack depth >= 12);
  * stack condition: the block of pop's LDS read carries no vmcnt wait, and none follows up to the node record's loads (the join of the branches
    included) -- the stack's scratch words are waited for inside their branch and nothing else in flight is the stack's.
The places are found through the line table (-gline-tables-only, as tools/isa_lines.py does); a second compilation without it, run at the same
time, shows that the line table leaves the instructions of both kernels as they are.  CPU-only: hipcc cross-compiles gfx950 without a GPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402  (HIPCC, DEVICE)

KERNELS = {"<true, true, false>": "k_trace_closestILb1ELb1ELb0E", "<true, false, false>": "k_trace_closestILb1ELb0ELb0E"}


def _command(out, line_table):
    return [isa_census.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"), "-I" + isa_census.DEVICE,
            "-Wno-unused-function", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-freciprocal-math", "-fapprox-func",  # (csrc/Makefile: PT_KERNELS_FP)
            "--cuda-device-only", "-S", "-o", out, os.path.join(isa_census.DEVICE, "pt_kernels.hip")] + (["-gline-tables-only"] if line_table else [])


def _source_lines(name, pattern, after=None):
    """1-based numbers of the lines of device/<name> that contain `pattern`, looking only behind the first line that contains `after`."""
    lines = open(os.path.join(isa_census.DEVICE, name)).read().split("\n")
    start = next(i for i, l in enumerate(lines) if after in l) if after else 0
    hits = [i + 1 for i, l in enumerate(lines) if i >= start and pattern in l]
    assert hits, (name, pattern)
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


def _vmcnt(ins):
    m = re.search(r"vmcnt\((\d+)\)", ins) if ins.startswith("s_waitcnt") else None
    return int(m.group(1)) if m else None


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa_census.HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("walk_overlap_isa")
    outs = [str(tmp / "lines.s"), str(tmp / "plain.s")]
    procs = [subprocess.Popen(_command(o, i == 0), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for i, o in enumerate(outs)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-2000:]
    with_lines, plain = (open(o).read() for o in outs)
    return {name: (_kernel(with_lines, mangled), _kernel(plain, mangled)) for name, mangled in KERNELS.items()}


TRI_LINE = ("pt_kernels.hip", _source_lines("pt_kernels.hip", "tr.T = sc.tris[", after="void triRoundPublish("))
NODE_LINE = ("pt_bvh8.h", _source_lines("pt_bvh8.h", "n0 = N[0]; n1 = N[1];", after="void bvh8Visit("))
NODE_LDS_LINE = ("pt_bvh8.h", _source_lines("pt_bvh8.h", "= N[0], b = N[1]", after="void bvh8Visit("))
POP_LDS_LINE = ("pt_bvh8.h", _source_lines("pt_bvh8.h", "uint32_t(lds[", after="NodeGroup pop()"))


def _at(entry, place):
    return entry[1] is not None and entry[1][0] == place[0] and entry[1][1] in place[1]


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_the_line_table_leaves_the_instructions_alone(compiled, name):
    with_lines, plain = compiled[name]
    assert [i[0] for i in with_lines] == [i[0] for i in plain]


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_no_wait_on_the_triangle_records_before_the_node_record_is_requested(compiled, name):
    k = compiled[name][0]
    tri = [i for i, e in enumerate(k) if e[0].startswith("global_load") and _at(e, TRI_LINE)]
    assert len(tri) >= 2 and len({k[i][2] for i in tri}) == 1, [k[i] for i in tri]  # the 48-byte record: one publish site, its loads in one block
    node = next(i for i, e in enumerate(k) if i > tri[-1] and e[0].startswith("global_load") and _at(e, NODE_LINE))
    issued, seen = 0, []
    for i in range(tri[0], node):
        ins, _, block = k[i]
        if i in tri:
            issued += 1
        n = _vmcnt(ins)
        if n is None:
            continue
        own_branch = any(k[j][2] == block and k[j][0].startswith("scratch_load") for j in range(tri[0], i))  # LaneStack2::pop, overflow branch
        seen.append((i - tri[0], ins, issued, own_branch))
        assert n >= issued or own_branch, (name, seen, [e[0] for e in k[tri[0]:i + 1]][-12:])
    print(name, "triangle loads", len(tri), "instructions up to the node record's loads", node - tri[0], "vmcnt waits on the way", seen)
    # ... and the first wait behind the node record's loads covers the triangle records: it leaves fewer loads in flight than the node record has
    node_loads = [i for i in range(node, len(k)) if k[i][2] == k[node][2] and k[i][0].startswith("global_load") and _at(k[i], NODE_LINE)]
    first = next(_vmcnt(k[i][0]) for i in range(node_loads[-1], len(k)) if _vmcnt(k[i][0]) is not None)
    assert first < len(node_loads), (first, len(node_loads))


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_the_lds_pop_path_carries_no_vector_memory_wait(compiled, name):
    k = compiled[name][0]
    pops = [i for i, e in enumerate(k) if e[0].startswith("ds_read") and _at(e, POP_LDS_LINE)]
    assert len(pops) >= 2, pops  # the node step is inlined behind a round and on its own
    for p in pops:
        first = next(i for i in range(p, -1, -1) if k[i][2] != k[p][2]) + 1
        in_block = [k[i][0] for i in range(first, p) if _vmcnt(k[i][0]) is not None]
        assert not in_block, (name, in_block)
        node = next(i for i in range(p, len(k)) if (k[i][0].startswith("global_load") and _at(k[i], NODE_LINE)) or (k[i][0].startswith("ds_read") and _at(k[i], NODE_LDS_LINE)))
        behind = [k[i][0] for i in range(p, node) if _vmcnt(k[i][0]) is not None]
        assert not behind, (name, behind)
