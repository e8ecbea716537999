"""The acceleration state of an instance (mi_pt_api.hip: the tree's arrays, the update mode, resident mode, the refit data and the counters),
characterised: scripted sequences of calls over three tiny scenes, and after EVERY call one record of what the instance reports -- the call's
outcome, mi_pt_get_accel_info, mi_pt_get_accel_resident_info, sceneBytes and the node / triangle-slot figures of the statistics.  The journal
is compared record by record with tests/golden/accel_state_journal.json, which was written by the library as it stood before the state got
an owner of its own (struct Accel): a change to that code that changes what an instance reports at any step shows up here.

Each step exists because a rule of that code lives there: the build of a switch to REFIT and the call that builds nothing, HOME refits, the
rebuild of a visibility change outside resident mode, AUTO's rebuild after a refit, the refit data going with REBUILD, visibility refits and
material patches in resident mode, in force against enabled, the empty state a failed build leaves (MI_PT_DIAG_FAIL_BUILD) and the build
after it, a scene with nothing visible -- where sceneBytes shows which arrays a rebuild releases at its head and which only when they are
next allocated --, the BVH2 walk (no refit data, resident mode inert) and the one-reference scene whose resident attempt falls back to a
plain build that counts once.  A step the library refuses is journalled as refused.

Nothing is rendered.  The SAH costs are exact doubles in the journal: two journals written by the same library were equal in every field.

`python tests/test_gpu_accel_state.py OUT.json` (the repository root on PYTHONPATH) writes the journal of the library in use."""
import ctypes as C
import json
import math
import os
import re
import sys

import numpy as np
import pytest

from vk_gltf_renderer_amd import _capi as capi
from vk_gltf_renderer_amd import pathtracer as ptmod
from vk_gltf_renderer_amd import scenegen

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "accel_state_journal.json")
FLOOR, SPHERE_A, SPHERE_B, SPHERE_C = range(4)  # render nodes of the spheres scene; A and B share one material
NUDGE = (0.25, 0.0, 0.0)
# the spheres towards three edges of the floor, at their height: the root box stays, every node that holds a sphere and something else grows
APART = {SPHERE_A: (-3.0, 0.0, 4.0), SPHERE_B: (0.0, 0.0, -4.5), SPHERE_C: (3.0, 0.0, 4.5)}


def _spheres(path):
    """A 4 x 4 floor grid and three small spheres under three nodes: two share `red`, the third has `green`, and `blue` is there to switch to."""
    b = scenegen.GlbBuilder()
    pos, nrm, uv, idx = scenegen.grid(4, 4, (10, 10), "y")
    b.node(mesh=b.mesh([b.primitive(pos, idx, nrm, uv, material=b.material(scenegen.lambert_material((0.5, 0.5, 0.5))))]))
    red, green = b.material(scenegen.lambert_material((0.8, 0.3, 0.2))), b.material(scenegen.lambert_material((0.2, 0.7, 0.3)))
    sp = scenegen.uv_sphere(12, 6, 0.6)
    for k, m in enumerate((red, red, green)):
        b.node(mesh=b.mesh([b.primitive(sp[0], sp[3], sp[1], sp[2], material=m)]), translation=[-1.5 + 1.5 * k, 0.61, 0.0])
    # the material to switch to hangs on a primitive of a mesh no node instantiates
    blue = b.material(scenegen.lambert_material((0.3, 0.3, 0.8)))
    b.mesh([b.primitive(sp[0], sp[3], sp[1], sp[2], material=blue)])
    b.camera_node((0.0, 2.5, 5.0), (0, 0.5, 0), yfov=0.7)
    return b.save(path), blue


def _one_triangle(path):
    b = scenegen.GlbBuilder()
    pos = np.array([[-1, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    nrm = np.array([[0, 0, 1]] * 3, np.float32)
    b.node(mesh=b.mesh([b.primitive(pos, np.array([0, 1, 2]), nrm, material=b.material(scenegen.lambert_material((0.5, 0.5, 0.5))))]))
    b.camera_node((0.0, 0.5, 3.0), (0, 0.5, 0), yfov=0.7)
    return b.save(path)


class _Driver:
    """One instance, its own copy of the node table and visibility flags, and the journal of its calls."""

    def __init__(self, scene, journal, env=None, **kw):
        self.journal, self.tr = journal, None
        d = scene.desc.contents
        self.n = int(d.numRenderNodes)
        self.nodes = (capi.MiGltfRenderNode * self.n)()
        C.memmove(self.nodes, d.renderNodes, C.sizeof(self.nodes))
        self.home = [list(self.nodes[i].objectToWorld) + list(self.nodes[i].worldToObject) for i in range(self.n)]
        self.vis = (C.c_uint8 * self.n)(*([1] * self.n))

        def create():  # (run-time switches are read once, at mi_pt_create)
            os.environ.update(env or {})
            try:
                self.tr = ptmod.PathTracer(scene, **kw)
            finally:
                for k in env or {}:
                    del os.environ[k]
        self.call("create", create)

    def call(self, step, fn):
        record = {"step": step, "outcome": "ok"}
        try:
            fn()
        except ptmod.MiError as e:
            rc, message = re.match(r"libmi_pt: rc=(-?\d+): (.*)", str(e), re.S).groups()
            record["outcome"] = {"rc": int(rc), "message": message}
        if self.tr is not None:
            a, s = self.tr.accel_info(), self.tr.stats()
            for k in ("sahCost", "sahCostAtBuild"):
                assert math.isfinite(a[k]) and a[k] >= 0.0, (step, a)
            record.update(accel=a, resident=self.tr.accel_resident_info(), sceneBytes=self.tr.memory()["sceneBytes"],
                          bvhNodeCount=s["bvhNodeCount"], bvhTriangleCount=s["bvhTriangleCount"], bvhNodeBytes=s["bvhNodeBytes"])
        self.journal.append(record)

    def update(self, step, hidden=None, moved=(), materials=()):
        """hidden: the set of hidden render nodes (None: no visibility array); moved: {node: (dx, dy, dz)} on top of the home matrices (pure
        translations in these scenes), every other node at home; materials: {node: material id}, which stays."""
        for i in range(self.n):
            self.nodes[i].objectToWorld[:] = self.home[i][:16]
            self.nodes[i].worldToObject[:] = self.home[i][16:]
        for i, delta in dict(moved).items():  # (column-major: elements 12 .. 14 are the translation)
            for c in range(3):
                self.nodes[i].objectToWorld[12 + c] += delta[c]
                self.nodes[i].worldToObject[12 + c] -= delta[c]
        for i, m in dict(materials).items():
            self.nodes[i].materialID = m
        for i in range(self.n):
            self.vis[i] = 0 if hidden and i in hidden else 1
        self.call(step, lambda: self.tr.update_render_nodes(self.nodes, self.n, None if hidden is None else self.vis))

    def mode(self, mode, ratio=1.5):
        self.call("set_accel_update(%s, %g)" % (mode, ratio), lambda: self.tr.set_accel_update(mode, ratio))

    def resident(self, on):
        self.call("set_accel_resident(%s)" % on, lambda: self.tr.set_accel_resident(on))

    def close(self):
        if self.tr is not None:
            self.tr.close()


def _modes(spheres, blue, triangle, j):
    d = _Driver(spheres, j, env={"MI_PT_REINSERT": "0"}, bvh=0)
    d.update("the same table: a build")
    d.mode("refit")  # the switch build
    d.mode("refit")  # no build
    d.update("move one node: a refit", moved={SPHERE_A: NUDGE})
    d.update("move it back: HOME", moved={})
    d.update("hide a node: a rebuild outside resident mode", hidden={SPHERE_B})
    d.update("show it", hidden=set())
    d.mode("auto", 1.0)
    d.update("a large move: a refit, then AUTO's rebuild", hidden=set(), moved=APART)
    d.mode("rebuild")  # the refit data goes
    d.close()


def _resident(spheres, blue, triangle, j):
    d = _Driver(spheres, j)
    d.mode("refit")
    d.resident(True)  # the switch build
    d.update("hide: a visibility refit", hidden={SPHERE_C})
    d.update("hide and move in one update", hidden={SPHERE_B, SPHERE_C}, moved={SPHERE_A: NUDGE})
    d.update("show", hidden=set(), moved={SPHERE_A: NUDGE})
    d.update("switch a material id: a patch", hidden=set(), moved={SPHERE_A: NUDGE}, materials={SPHERE_C: blue})
    d.update("an update that changes nothing", hidden=set(), moved={SPHERE_A: NUDGE})
    d.mode("rebuild")  # out of force, still enabled
    d.mode("refit")
    d.resident(False)
    d.close()


def _failure(refit):
    def run(spheres, blue, triangle, j):
        d = _Driver(spheres, j, env={"MI_PT_DIAG_FAIL_BUILD": "3"})
        if refit:
            d.mode("refit")
        d.update("visibility change 1", hidden={SPHERE_A})
        d.update("visibility change 2", hidden=set())
        d.update("visibility change 3", hidden={SPHERE_B})
        d.mode("refit")
        d.update("an update", hidden={SPHERE_B})
        d.close()
    return run


def _nothing_visible(resident):
    def run(spheres, blue, triangle, j):
        d = _Driver(spheres, j)
        if resident:
            d.mode("refit")
            d.resident(True)
        d.update("hide every node", hidden=set(range(d.n)))
        d.update("show them", hidden=set())
        d.close()
    return run


def _bvh2_walk(spheres, blue, triangle, j):
    d = _Driver(spheres, j, bvh=1)
    d.mode("refit")  # no build, no refit data
    d.resident(True)  # inert
    d.update("move", moved={SPHERE_A: NUDGE})
    d.update("hide", hidden={SPHERE_B}, moved={SPHERE_A: NUDGE})
    d.close()


def _one_reference(spheres, blue, triangle, j):
    d = _Driver(triangle, j)
    d.mode("refit")
    d.resident(True)
    d.update("hide the only node: the resident attempt falls back, one build", hidden={0})
    d.update("show it", hidden=set())
    d.close()


SEQUENCES = {"A modes": _modes, "B resident": _resident, "C failure, REFIT": _failure(True), "C failure, REBUILD": _failure(False),
             "D nothing visible, REBUILD": _nothing_visible(False), "D nothing visible, resident": _nothing_visible(True), "E BVH2 walk": _bvh2_walk,
             "F one reference": _one_reference}


def _scenes(tmp):
    path, blue = _spheres(os.path.join(str(tmp), "spheres.glb"))
    spheres, triangle = ptmod.Scene(path), ptmod.Scene(_one_triangle(os.path.join(str(tmp), "triangle.glb")))
    d = spheres.desc.contents
    assert d.numRenderNodes == 4 and d.numMaterials == 4 and blue == 3, (d.numRenderNodes, d.numMaterials, blue)
    assert [d.renderNodes[i].materialID for i in range(4)] == [0, 1, 1, 2]
    assert triangle.desc.contents.numRenderNodes == 1
    return spheres, blue, triangle


def _journal(tmp, name):
    records = []
    SEQUENCES[name](*_scenes(tmp), records)
    return json.loads(json.dumps(records))  # (as the golden file holds it; a double survives the round trip exactly)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_these_sequences(golden):
    assert sorted(golden) == sorted(SEQUENCES)


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_journal_equals_the_one_recorded_before_the_state_had_an_owner(name, golden, tmp_path):
    got, want = _journal(tmp_path, name), golden[name]
    for k, (g, w) in enumerate(zip(got, want)):
        print(name, k, json.dumps(g))
        assert g == w, (name, k, g["step"], {f: (g.get(f), w.get(f)) for f in set(g) | set(w) if g.get(f) != w.get(f)})
    assert len(got) == len(want), (name, len(got), len(want))


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = {name: _journal(tmp, name) for name in sorted(SEQUENCES)}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
