"""Adversarial geometry through every configuration of the acceleration-structure builder, black box: per case of tests/builder_cases.py one
instance per configuration below, the case's 1024 rays through mi_pt_query_rays, closed again.

  A  bvh 0                                      F  bvh 0, MI_PT_COLLAPSE=greedy, MI_PT_HOST_COLLAPSE=1
  B  bvh 1  (the BVH2 walk)                     G  bvh 0, MI_PT_REINSERT=0
  C  bvh 2  (Karras topology, 8-wide walk)      H  bvh 1, MI_PT_REINSERT=0
  D  bvh 3  (Karras topology, BVH2 walk)        I  bvh 0, MI_PT_SPLIT=1, MI_PT_SPLIT_MIN_SHARE=0, MI_PT_SPLIT_DEPTH=10
  E  bvh 0, MI_PT_COLLAPSE=greedy               J  bvh 1, the switches of I

A's closest hits against the float64 brute force of tests/query_util.py (exact ids on the unambiguous rays, t and barycentrics within 8 x the
float32 error builder_cases.MEASURED records: tests/test_builder_cases_reference.py checks those figures and the cases' properties on the CPU);
the records of B .. J equal A's byte for byte -- a tree decides what a walk visits, never what it returns; ANY agrees with CLOSEST on hit / miss
in A, B and D.

The chains (130 / 600 nested corner triangles) are what PLOC clusters into a BVH2 as deep as its leaves are many -- and what reinsertion turns the
Karras tree into as well; a ray from inside leaves one stack entry per level.  Before the builder bounded the height of the tree it hands a walk
(buildBvh) the BVH2 walk dropped what its 96 entries could not hold and ended at the first pop from the dropped range: of
1024 rays B and H missed 187 (chain130) / 441 (chain600), J missed 9 / 410 and returned another shell on 92 / 0, D -- no miss -- returned another
shell than the nearest on 83 / 427; the six 8-wide configurations were right throughout (a node with one inner child pushes nothing).  Every other case
passed as it was.  Figures per case: LABNOTES.md, "Adversarial geometry through every builder configuration"."""
import numpy as np
import pytest

import builder_cases as bc
import query_util as qu
from test_gpu_query import _environment
from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod

pytestmark = pytest.mark.gpu
HIT = capi.MI_PT_HIT
SPLIT = {"MI_PT_SPLIT": "1", "MI_PT_SPLIT_MIN_SHARE": "0", "MI_PT_SPLIT_DEPTH": "10"}
CONFIGURATIONS = (("A", 0, {}), ("B", 1, {}), ("C", 2, {}), ("D", 3, {}), ("E", 0, {"MI_PT_COLLAPSE": "greedy"}),
                  ("F", 0, {"MI_PT_COLLAPSE": "greedy", "MI_PT_HOST_COLLAPSE": "1"}), ("G", 0, {"MI_PT_REINSERT": "0"}), ("H", 1, {"MI_PT_REINSERT": "0"}),
                  ("I", 0, SPLIT), ("J", 1, SPLIT))


@pytest.mark.parametrize("name", bc.NAMES)
def test_builder_matrix(tmp_path, name):
    scene = ptmod.Scene(bc.make_scene(name, tmp_path))
    st = qu.SceneTris(scene, nodes=bc.reference_nodes(name))
    rays = bc.make_rays(name, st)
    ref = qu.Reference(qu.Pairs(st, rays))
    assert float(ref.ambiguous.mean()) <= qu.MAX_AMBIGUOUS_SHARE  # (before anything of the GPU's is looked at)
    rows = qu.as_rows(rays)
    closest, differing = {}, {}
    for cfg, bvh, switches in CONFIGURATIONS:
        with _environment(switches):
            tr = ptmod.PathTracer(scene, bvh=bvh)
        try:
            got = closest[cfg] = tr.query_rays(rows)
            hit = (got["flags"] & HIT) != 0
            slots = tr.stats()["bvhTriangleCount"]
            differing[cfg] = int((got.view(np.uint8).reshape(-1, 64) != closest["A"].view(np.uint8).reshape(-1, 64)).any(1).sum())
            print("BUILDERMATRIX", name, cfg, "slots", slots, "hits", int(hit.sum()), "of", int(ref.hit.sum()), "in the reference; misses where it hits:",
                  int((ref.hit & ~ref.ambiguous & ~hit).sum()), "records differing from A:", differing[cfg])
            if cfg in ("A", "B", "D"):
                a = tr.query_rays(rows, mode="any")
                assert (((a["flags"] & HIT) != 0) == hit).all(), (cfg, "ANY disagrees with CLOSEST on hit / miss")
                assert (a["renderNode"][~hit] == -1).all() and (a["flags"][~hit] == 0).all(), cfg
                assert (a["t"][hit] >= got["t"][hit]).all(), cfg
            if cfg == "A" and name.startswith("counts_"):
                assert slots == int(name[7:]) == scene.num_triangles
            if cfg in ("I", "J") and name == "needles":
                assert slots > scene.num_triangles, (cfg, slots)  # references really are in the tree
        finally:
            tr.close()
    # (a hit position is rounded to float32 where it lies: half an ulp of its largest coordinate, 2^-24 of it, on top of what t's error moves it --
    #  `offset`, 2^16 from the origin: 0.0039 against 0.0009)
    qu.check_hits(st, rays, ref, closest["A"], *bc.TOLERANCE[name], what=name + " (A)", position_rounding=2.0 ** -24 * float(np.abs(ref.position).max()))
    assert not any(differing.values()), differing
    scene.close()
