"""Skins and morph targets on the host (csrc/host/gltf_scene_animation.cpp, mi_scene_deformation / mi_scene_deform_on_host): the tables
the front end builds from scenegen.scene_skinned are compared with an independent numpy reading of the glTF 2.0 rules (tests/deform_util.py)
at several clip times -- decoded influences in every component type, sparse deltas, joint matrices, morph weights of LINEAR / STEP /
CUBICSPLINE weights channels -- and the host deformation with the two shaders restated in numpy.  CPU only."""
import os

import numpy as np
import pytest

import deform_util as du
from vk_gltf_renderer_amd import scenegen

TIMES = (0.0, 0.4, 1.25, 1.7, 2.3, 2.95)


@pytest.fixture(scope="module")
def skinned(tmp_path_factory):
    return scenegen.scene_skinned(str(tmp_path_factory.mktemp("deform") / "skinned.glb"))


def _scene(path):
    from vk_gltf_renderer_amd.pathtracer import Scene
    return Scene(path)


def _gltf_prims(doc):
    """(mesh, primitive) of every render primitive, in creation order (scene_skinned shares no primitive between meshes)."""
    return [(m, p) for m, mesh in enumerate(doc["meshes"]) for p in range(len(mesh["primitives"]))]


def _first_users(doc, gp):
    """render primitive -> the first node (traversal order) that draws it"""
    users = {}

    def visit(n):
        node = doc["nodes"][n]
        if "mesh" in node:
            for k in range(len(doc["meshes"][node["mesh"]]["primitives"])):
                users.setdefault(gp.index((node["mesh"], k)), n)
        for c in node.get("children", []):
            visit(c)
    for r in doc["scenes"][0]["nodes"]:
        visit(r)
    return users


def test_tables_follow_the_gltf_rules(built, skinned):
    doc, blob = du.load_glb(skinned)
    sc = _scene(skinned)
    d = sc.deformation
    assert d is not None and d.numPrims == 4
    gp = _gltf_prims(doc)
    users = _first_users(doc, gp)
    by_prim = {p.renderPrimID: p for p in du.prims(d)}
    types = set()
    for rp, p in by_prim.items():
        mesh, k = gp[rp]
        gprim = doc["meshes"][mesh]["primitives"][k]
        assert p.vertexCount == len(du.accessor(doc, blob, gprim["attributes"]["POSITION"]))
        if "JOINTS_0" in gprim["attributes"]:
            j = du.accessor(doc, blob, gprim["attributes"]["JOINTS_0"]).astype(np.int64)
            w = du.accessor(doc, blob, gprim["attributes"]["WEIGHTS_0"])
            types.add(doc["accessors"][gprim["attributes"]["JOINTS_0"]]["componentType"])
            types.add(doc["accessors"][gprim["attributes"]["WEIGHTS_0"]]["componentType"] + 100)
            assert (du.arr(p.joints, p.vertexCount * 4, np.int64).reshape(-1, 4) == j).all()
            assert np.allclose(du.arr(p.weights, p.vertexCount * 4).reshape(-1, 4), w, atol=1e-7)
            assert p.numJoints == len(doc["skins"][doc["nodes"][users[rp]]["skin"]]["joints"])
        else:
            assert not p.joints and not p.weights
        targets = gprim.get("targets", [])
        assert p.numTargets == len(targets)
        if targets:
            dp = du.arr(p.positionDeltas, p.vertexCount * 3 * len(targets)).reshape(len(targets), -1, 3)
            for t, tg in enumerate(targets):
                assert np.allclose(dp[t], du.accessor(doc, blob, tg["POSITION"]), atol=1e-7), t  # (sparse ones included)
            assert bool(p.normalDeltas) == any("NORMAL" in tg for tg in targets)
    assert types == {5121, 5123, 5126 + 100, 5121 + 100, 5123 + 100}  # u8 / u16 joints; float, unorm8, unorm16 weights
    # the sparse targets decode: only the patch moves in target 1; target 2 = its dense base with three vertices overridden
    blob_prim = by_prim[gp.index((2, 0))]
    dp = du.arr(blob_prim.positionDeltas, blob_prim.vertexCount * 9).reshape(3, -1, 3)
    moved = np.nonzero(np.abs(dp[1]).sum(1))[0]
    assert 0 < len(moved) < blob_prim.vertexCount // 4 and np.allclose(dp[1][moved], [0.25, 0, 0])
    # frame tables at several times (LINEAR, STEP and CUBICSPLINE weights channels cover [0, 1], [1, 2], [2, 3])
    for time in TIMES:
        assert sc.update_animation(0, time)
        world, weights = du.pose(doc, blob, 0, time)
        jt, mw = du.frame_tables(d)
        for rp, p in by_prim.items():
            if p.joints:
                node = users[rp]
                exp = du.joint_matrices(doc, blob, world, doc["nodes"][node]["skin"], node)
                got = jt[p.jointMatrixOffset:p.jointMatrixOffset + p.numJoints].reshape(-1, 4, 4).transpose(0, 2, 1)
                for g, e in zip(got, exp):
                    assert np.abs(g - e).max() <= 1e-5 * max(1.0, np.abs(e).max()), (time, rp)
            if p.numTargets:
                mesh = gp[rp][0]
                exp = np.zeros(p.numTargets)
                exp[:min(p.numTargets, len(weights[mesh]))] = weights[mesh][:p.numTargets]
                assert np.allclose(mw[p.morphWeightOffset:p.morphWeightOffset + p.numTargets], exp, atol=1e-6), (time, rp)
    sc.close()


def test_deform_on_host_matches_the_shaders(built, skinned):
    sc = _scene(skinned)
    d = sc.deformation
    desc = sc.desc.contents
    rest = {p.renderPrimID: du.arr(desc.renderPrimitives[p.renderPrimID].positions, p.vertexCount * 3) for p in du.prims(d)}
    for time in (0.7, 2.6):
        sc.update_animation(0, time)
        jt, mw = du.frame_tables(d)
        assert sc.deform_on_host() == 4
        for p in du.prims(d):
            rp = desc.renderPrimitives[p.renderPrimID]
            ep, en, et = du.deform_reference(p, jt, mw, np.float64)
            gpos = du.arr(rp.positions, p.vertexCount * 3).reshape(-1, 3)
            assert np.abs(gpos - ep).max() <= 2e-6 * max(1.0, np.abs(ep).max()), (time, p.renderPrimID)
            assert not np.array_equal(gpos.reshape(-1), rest[p.renderPrimID])
            if en is not None:
                assert np.abs(du.arr(rp.normals, p.vertexCount * 3).reshape(-1, 3) - en).max() < 1e-5
            if et is not None:
                gt = du.arr(rp.tangents, p.vertexCount * 4).reshape(-1, 4)
                assert np.abs(gt[:, :3] - et[:, :3]).max() < 1e-5
                assert np.array_equal(gt[:, 3], du.arr(p.baseTangents, p.vertexCount * 4).reshape(-1, 4)[:, 3])  # w kept
    sc.close()


def test_zero_morph_weights_leave_a_morph_only_primitive_bit_identical(built, skinned):
    sc = _scene(skinned)
    d = sc.deformation
    sc.update_animation(0, 0.0)  # the blob's weights are all zero at t = 0
    _, mw = du.frame_tables(d)
    blob = [p for p in du.prims(d) if p.numTargets == 3][0]
    assert not blob.joints and not mw[blob.morphWeightOffset:blob.morphWeightOffset + 3].any()
    sc.deform_on_host()
    rp = sc.desc.contents.renderPrimitives[blob.renderPrimID]
    assert np.array_equal(du.arr(rp.positions, blob.vertexCount * 3), du.arr(blob.basePositions, blob.vertexCount * 3))
    sc.close()


def test_tables_survive_mikktspace_splitting(built, skinned):
    sc = _scene(skinned)
    before = {p.renderPrimID: (p.vertexCount, du.arr(p.joints, p.vertexCount * 4, np.int64) if p.joints else None) for p in du.prims(sc.deformation)}
    assert sc.recompute_tangents(force_creation=True, mikktspace=True) > 0
    d = sc.deformation
    desc = sc.desc.contents
    grew = 0
    for p in du.prims(d):
        rp = desc.renderPrimitives[p.renderPrimID]
        assert p.vertexCount == rp.vertexCount
        assert np.array_equal(du.arr(p.basePositions, p.vertexCount * 3), du.arr(rp.positions, p.vertexCount * 3))
        n0, j0 = before[p.renderPrimID]
        if p.vertexCount == n0:
            continue
        grew += 1
        pos = du.arr(rp.positions, p.vertexCount * 3).reshape(-1, 3)
        same = [np.nonzero((pos[:n0] == pos[v]).all(1))[0] for v in range(n0, p.vertexCount)]
        if p.joints:  # every added vertex carries the influences of an original vertex at the same place
            j = du.arr(p.joints, p.vertexCount * 4, np.int64).reshape(-1, 4)
            assert np.array_equal(j[:n0].reshape(-1), j0)
            for v, s in zip(range(n0, p.vertexCount), same):
                assert any((j[k] == j[v]).all() for k in s), v
        if p.numTargets:
            dp = du.arr(p.positionDeltas, p.vertexCount * 3 * p.numTargets).reshape(p.numTargets, -1, 3)
            for v, s in zip(range(n0, p.vertexCount), same):
                assert any((dp[:, k] == dp[:, v]).all() for k in s), v
    assert grew > 0
    sc.update_animation(0, 1.3)
    jt, mw = du.frame_tables(d)
    sc.deform_on_host()
    for p in du.prims(d):
        ep, _, _ = du.deform_reference(p, jt, mw, np.float64)
        gpos = du.arr(desc.renderPrimitives[p.renderPrimID].positions, p.vertexCount * 3).reshape(-1, 3)
        assert np.abs(gpos - ep).max() <= 2e-6 * max(1.0, np.abs(ep).max())
    sc.close()


def _masked_skinned(tmp_path):
    """A skinned alpha-MASK quad and the same quad unskinned."""
    b = scenegen.GlbBuilder()
    tex = np.zeros((16, 16, 4), np.uint8)
    tex[..., :3] = 200
    tex[:8, :, 3] = 255  # half of the texture is empty: the cut drops triangles there
    mat = b.material({"pbrMetallicRoughness": {"baseColorTexture": {"index": b.texture(b.image(tex), b.sampler(9728, 9728))}}, "alphaMode": "MASK"})
    pos, nrm, uv, idx = scenegen.grid(4, 4)
    j = np.zeros((len(pos), 4), np.uint8)
    w = np.zeros((len(pos), 4), np.float32)
    w[:, 0] = 1
    joint = b.node(root=False)
    skin = b.skin([joint])
    skinned = b.mesh([b.primitive(pos, idx, nrm, uv, material=mat, joints=j, weights=w)])
    plain = b.mesh([b.primitive(pos + 0.01, idx, nrm, uv, material=mat)])
    b.node(mesh=skinned, skin=skin)
    b.node(mesh=plain)
    b.node(children=[joint])
    return b.save(str(tmp_path / "masked.glb"))


def test_cut_alpha_leaves_deforming_primitives_whole(built, tmp_path):
    sc = _scene(_masked_skinned(tmp_path))
    d = sc.deformation
    assert d is not None and d.numPrims == 1
    skinned = d.prims[0].renderPrimID
    desc = sc.desc.contents
    tris = [desc.renderPrimitives[i].triangleCount for i in range(desc.numRenderPrimitives)]
    assert sc.cut_alpha(4) > 0
    desc = sc.desc.contents
    after = [desc.renderPrimitives[i].triangleCount for i in range(desc.numRenderPrimitives)]
    assert after[skinned] == tris[skinned]
    assert any(after[i] != tris[i] for i in range(len(tris)) if i != skinned)
    sc.close()


def _tiny(tmp_path, name, edit):
    """A skinned quad (two influences on one joint) and a morphed quad with 2 targets, a joint channel and a weights channel."""
    b = scenegen.GlbBuilder()
    pos, nrm, uv, idx = scenegen.grid(2, 2)
    j = np.zeros((len(pos), 4), np.uint8)
    j[:, 1] = 1
    w = np.tile(np.array([[0.5, 0.5, 0, 0]], np.float32), (len(pos), 1))
    mat = b.material(scenegen.lambert_material())
    joint = b.node(root=False, translation=[0, 0.5, 0])
    skin = b.skin([joint, joint], np.stack([np.eye(4)] * 2))
    sk_mesh = b.mesh([b.primitive(pos, idx, nrm, uv, material=mat, joints=j, weights=w)])
    mo_mesh = b.mesh([b.primitive(pos, idx, nrm, uv, material=mat, targets=[{"POSITION": nrm * 0.3}, {"POSITION": pos * 0.2}])], weights=[0.0, 0.0])
    sk_node = b.node(mesh=sk_mesh, skin=skin, children=[joint])
    mo_node = b.node(mesh=mo_mesh, translation=[2, 0, 0])
    b.animation([(joint, "translation", [0.0, 1.0], [[0, 0.5, 0], [0, 1.0, 0.3]], "LINEAR"),
                 (mo_node, "weights", [0.0, 1.0], [[0.0, 0.0], [1.0, 0.5]], "LINEAR")])
    edit(b, dict(joint=joint, skin=skin, sk_node=sk_node, mo_node=mo_node, n=len(pos)))
    return b.save(str(tmp_path / name))


def test_hostile_files_load_and_keep_their_base_pose(built, tmp_path):
    """Scene files are untrusted: every damaged deformation input loads, evaluates without a crash or a non-finite table entry, and the
    geometry at load is the file's base pose."""
    def joints_beyond_skin(b, k):
        b.doc["meshes"][0]["primitives"][0]["attributes"]["JOINTS_0"] = b.accessor(np.full((k["n"], 4), 9, np.uint8), 34962)

    def short_ibm(b, k):
        b.doc["skins"][0]["inverseBindMatrices"] = b.accessor(np.eye(4, dtype=np.float32).reshape(1, 16))

    def weights_count_mismatch(b, k):
        b.doc["animations"][0]["samplers"][1]["output"] = b.accessor(np.linspace(0, 1, 10).astype(np.float32))  # 5 per key, 2 targets

    def nan_keys(b, k):
        b.doc["animations"][0]["samplers"][1]["output"] = b.accessor(np.array([np.nan, 0, 1, np.nan], np.float32))

    def no_joints(b, k):
        del b.doc["meshes"][0]["primitives"][0]["attributes"]["JOINTS_0"]

    def bad_skin_refs(b, k):
        b.doc["skins"][0]["joints"] = [99, -4]

    def skin_out_of_range(b, k):
        b.doc["nodes"][k["sk_node"]]["skin"] = 7

    def short_target(b, k):
        t = b.doc["meshes"][1]["primitives"][0]["targets"][0]
        b.doc["accessors"][t["POSITION"]]["count"] = 2

    for name, edit in [("beyond", joints_beyond_skin), ("ibm", short_ibm), ("wcount", weights_count_mismatch), ("nan", nan_keys),
                       ("nojoints", no_joints), ("refs", bad_skin_refs), ("skinrange", skin_out_of_range), ("shorttarget", short_target)]:
        path = _tiny(tmp_path, name + ".glb", edit)
        doc, blob = du.load_glb(path)
        sc = _scene(path)
        desc = sc.desc.contents
        gprims = [p for m in doc["meshes"] for p in m["primitives"]]
        for i, prim in enumerate(gprims):
            rp = desc.renderPrimitives[i]
            assert np.array_equal(du.arr(rp.positions, rp.vertexCount * 3), du.accessor(doc, blob, prim["attributes"]["POSITION"]).astype(np.float32).reshape(-1)), name
        for time in (0.0, 0.5, 1.0):
            sc.update_animation(0, time)
            d = sc.deformation
            if d is not None:
                jt, mw = du.frame_tables(d)
                assert np.isfinite(jt).all() and np.isfinite(mw).all(), name
                sc.deform_on_host()
        d = sc.deformation
        if name in ("nojoints", "skinrange"):
            assert d is not None and all(not p.joints for p in du.prims(d)), name  # (the morphed quad remains)
        if name == "beyond":  # every influence names a joint beyond the skin: skipped, the vertices skin to the origin
            p = [p for p in du.prims(d) if p.joints][0]
            assert not du.arr(sc.desc.contents.renderPrimitives[p.renderPrimID].positions, p.vertexCount * 3).any()
        if name == "wcount":
            p = [p for p in du.prims(d) if p.numTargets][0]
            assert p.numTargets == 2 and d.numMorphWeights == 2
        sc.close()


def test_a_scene_without_deformers_has_no_tables(built, assets):
    sc = _scene(os.path.join(assets, "Box.glb"))
    assert sc.deformation is None and sc.deform_on_host() == 0
    sc.close()


def test_deformation_entry_points_refuse_a_null_instance(built):
    from vk_gltf_renderer_amd import _capi as capi
    if not os.path.exists(os.path.join(capi.LIB_DIR, "libmi_pt.so")):
        pytest.skip("libmi_pt.so not built yet")
    lib = capi.pt_lib()
    assert lib.mi_pt_set_deformation(None, None) == -1
    assert lib.mi_pt_update_deformation(None, None, None, 0) == -1
    assert lib.mi_pt_read_vertices(None, 0, None, None, None) == -1
