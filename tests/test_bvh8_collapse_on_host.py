"""The host collapse of the 8-wide BVH (csrc/device/bvh8_collapse_host.h: what the builder runs behind MI_PT_HOST_COLLAPSE=1 and for a
one-triangle scene) compiled for the host through tests/host_shim (g++ -ffp-contract=off) -- no GPU needed.  It collapses BVH2s written in numpy
in the record layout of bvh_build.hip, and the node array is held to the contract the header comment of bvh8.hip states: the permutation is one,
node 0 is the root, inner children lie contiguously from childBase and leaf triangles from triBase, both in slot order, imask and valid claim
disjoint slots, a leaf child has one or two triangles, an empty slot is 255 / 0, every used slot's decoded box fmaf(q, 2^(e - 127), p) -- in
float32 -- contains the union of the input boxes below it, and numLevels is the longest root path."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_bvh_refit_on_host import NODE8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_shim_collapse") / "libcollapse_on_host.so")
    shim = os.path.join(ROOT, "tests", "host_shim")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + shim,
                    "-I" + os.path.join(ROOT, "vk_gltf_renderer_amd", "csrc", "device"), "-I" + os.path.join(ROOT, "include"), "-o", out,
                    os.path.join(shim, "collapse_on_host.cpp")], check=True)
    L = C.CDLL(out)
    VP = C.c_void_p
    L.collapse_on_host.argtypes = [VP, C.c_int, C.c_uint32, C.c_uint32, VP, VP, VP, VP, VP]
    L.collapse_on_host.restype = C.c_int
    return L


# ---- BVH2s in numpy: a topology is a leaf index or a pair of topologies ---------------------------------------------------------------------------
def bvh2(topology, lo, hi):
    """(records (numInner, 4, 4) float32, root) of `topology` over the leaf boxes [lo, hi]: inner nodes numbered in post-order (the root last, as
    the clustering builder leaves it), child references >= 0 inner / ~leaf, triangle counts in [3][2]."""
    records = []

    def visit(t):  # -> (reference, lo, hi, count)
        if not isinstance(t, tuple):
            return ~int(t), lo[t], hi[t], 1
        kids = [visit(c) for c in t]
        rec = np.zeros((4, 4), F32)
        for k, (_, l, h, _) in enumerate(kids):
            rec[k] = (l[0], h[0], l[1], h[1])
            rec[2, 2 * k:2 * k + 2] = (l[2], h[2])
        rec[3].view(np.int32)[:3] = (kids[0][0], kids[1][0], kids[0][3] + kids[1][3])
        records.append(rec)
        return len(records) - 1, np.minimum(kids[0][1], kids[1][1]), np.maximum(kids[0][2], kids[1][2]), kids[0][3] + kids[1][3]

    root = visit(topology)[0]
    return np.array(records, F32).reshape(-1, 4, 4), root


def balanced(ids):
    ids = list(ids)
    return ids[0] if len(ids) == 1 else (balanced(ids[:len(ids) // 2]), balanced(ids[len(ids) // 2:]))


def random_topology(rng, ids):
    ids = list(ids)
    if len(ids) == 1:
        return ids[0]
    cut = int(rng.integers(1, len(ids)))
    return (random_topology(rng, ids[:cut]), random_topology(rng, ids[cut:]))


def random_boxes(rng, n, flat_axis=None):
    c = rng.uniform(-4.0, 4.0, size=(n, 3))
    h = rng.uniform(0.01, 0.5, size=(n, 3))
    lo, hi = (c - h).astype(F32), (c + h).astype(F32)
    if flat_axis is not None:
        lo[:, flat_axis] = hi[:, flat_axis] = F32(1.25)
    return lo, hi


def cases():
    rng = np.random.default_rng(8)
    lo, hi = random_boxes(rng, 1)
    yield "one triangle", None, lo, hi
    lo, hi = random_boxes(rng, 2)
    yield "two triangles", (0, 1), lo, hi
    lo, hi = random_boxes(rng, 9)
    yield "balanced over 9", balanced(range(9)), lo, hi
    s = np.array([F32(1.05 ** k) for k in range(41)], F32)  # 41 nested boxes [0, s]^3: 40 inner nodes, one below the other
    chain = 0
    for k in range(1, 41):
        chain = (chain, k)
    yield "chain of 40", chain, np.zeros((41, 3), F32), np.repeat(s[:, None], 3, 1)
    lo, hi = random_boxes(rng, 64, flat_axis=2)
    yield "flat set of 64", balanced(rng.permutation(64)), lo, hi
    for seed in (1, 2, 3):
        r = np.random.default_rng(seed)
        lo, hi = random_boxes(r, 64)
        yield "random topology %d over 64" % seed, random_topology(r, r.permutation(64)), lo, hi


CASES = list(cases())


def collapse(lib, topology, lo, hi):
    n = len(lo)
    records, root = (np.zeros((0, 4, 4), F32), ~0) if topology is None else bvh2(topology, lo, hi)
    assert len(records) == n - 1
    nodes = np.zeros(max(len(records), 1), NODE8)
    perm = np.full(n, 0xffffffff, np.uint32)
    levels = C.c_uint32(0)
    lone_lo, lone_hi = np.ascontiguousarray(lo[0]), np.ascontiguousarray(hi[0])
    count = lib.collapse_on_host(records.ctypes.data, root, len(records), n, lone_lo.ctypes.data, lone_hi.ctypes.data, nodes.ctypes.data,
                                 perm.ctypes.data, C.byref(levels))
    assert count >= 1, "the collapse lost triangles"
    return nodes[:count], perm, int(levels.value)


def f32_of(x):
    """The float32 nearest the exact number x (ties to even): what one fmaf returns."""
    f = F32(float(x))
    near = [np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))]
    return min(near, key=lambda c: (abs(Fraction(float(c)) - x), int(c.view(np.uint32)) & 1))


def decoded(node, axis, slot):
    scale = Fraction(2) ** (int(node["e"][axis]) - 127)
    p = Fraction(float(node["p"][axis]))
    return f32_of(int(node["qlo"][axis][slot]) * scale + p), f32_of(int(node["qhi"][axis][slot]) * scale + p)


@pytest.mark.parametrize("name,topology,lo,hi", CASES, ids=[c[0] for c in CASES])
def test_collapse_keeps_the_contract(lib, name, topology, lo, hi):
    n = len(lo)
    nodes, perm, levels = collapse(lib, topology, lo, hi)
    assert sorted(perm.tolist()) == list(range(n)), "the permutation is none"
    visited = []

    def check(index, depth):  # -> (triangles below node `index`, longest path from it)
        visited.append(index)
        node = nodes[index]
        imask, valid = int(node["imask"]), int(node["valid"])
        child, tri, below, longest = int(node["childBase"]), int(node["triBase"]), [], 1
        for slot in range(8):
            inner, v = (imask >> slot) & 1, (valid >> (2 * slot)) & 3
            assert not (inner and v), (name, index, slot, "imask and valid claim the slot")
            assert v in (0, 1, 3), (name, index, slot, "a leaf child has one or two triangles")
            if inner:
                assert child < len(nodes) and child > index, (name, index, slot)
                mine, path = check(child, depth + 1)  # (children in slot order take childBase, childBase + 1, ...)
                child += 1
                longest = max(longest, 1 + path)
            elif v:
                count = 2 if v == 3 else 1
                mine = [int(t) for t in perm[tri:tri + count]]  # (... and leaf triangles triBase, triBase + 1, ...)
                assert len(mine) == count, (name, index, slot)
                tri += count
            else:
                assert (node["qlo"][:, slot] == 255).all() and (node["qhi"][:, slot] == 0).all(), (name, index, slot, "an empty slot is 255 / 0")
                continue
            for axis in range(3):
                dlo, dhi = decoded(node, axis, slot)
                assert dlo <= lo[mine, axis].min() and dhi >= hi[mine, axis].max(), (name, index, slot, axis, "the decoded box does not contain its boxes")
            below += mine
        assert below, (name, index, "a node without children")
        return below, longest

    below, longest = check(0, 0)
    assert sorted(below) == list(range(n)), "node 0 is not the root of every triangle"
    # breadth-first, contiguous children: every node is reached once, and the indices a level hands out are consecutive
    assert sorted(visited) == list(range(len(nodes)))
    order = [0]
    for index in order:
        kids = bin(int(nodes[index]["imask"])).count("1")
        assert int(nodes[index]["childBase"]) == len(order) or kids == 0, (name, index, "children are not contiguous from childBase")
        order += range(len(order), len(order) + kids)
    tri = 0
    for node in nodes:  # leaf triangles are handed out node by node as well
        v = int(node["valid"])
        held = sum((1, 2)[((v >> (2 * s)) & 3) == 3] for s in range(8) if (v >> (2 * s)) & 3)
        assert int(node["triBase"]) == tri or held == 0, (name, "triangles are not contiguous from triBase")
        tri += held
    assert tri == n
    assert levels == longest, (name, levels, longest)


def test_chain_is_as_deep_as_the_collapse_allows(lib):
    """The chain has one inner BVH2 child per node: an 8-wide node opens it seven times, so 40 nested nodes make a path of more than one node."""
    _, topology, lo, hi = CASES[3]
    nodes, _, levels = collapse(lib, topology, lo, hi)
    assert levels == len(nodes) > 1
