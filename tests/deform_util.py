"""Independent numpy restatement of the glTF 2.0 rules for skins and morph targets (specification 3.7.3, 3.8, 3.11, appendix C), used by
the deformation tests: reads a .glb written by scenegen, evaluates a clip at a time (node TRS and mesh weights), and computes the joint
matrices inverse(world[refNode]) * world[joint] * IBM and the posed vertices the device kernel (csrc/device/deform.hip) must produce."""
import ctypes as C
import json
import struct

import numpy as np

_NC = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}
_DT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}


def load_glb(path):
    data = open(path, "rb").read()
    jlen = struct.unpack_from("<I", data, 12)[0]
    return json.loads(data[20:20 + jlen]), data[20 + jlen + 8:]


def accessor(doc, blob, index):
    """(count, components) float64, normalisation and sparse blocks applied."""
    acc = doc["accessors"][index]
    nc, dt, n = _NC[acc["type"]], np.dtype(_DT[acc["componentType"]]), acc["count"]
    out = np.zeros((n, nc), np.float64)
    if "bufferView" in acc:
        bv = doc["bufferViews"][acc["bufferView"]]
        out = np.frombuffer(blob, dt, n * nc, bv["byteOffset"] + acc.get("byteOffset", 0)).reshape(n, nc).astype(np.float64)
    if "sparse" in acc:
        sp = acc["sparse"]
        ib, vb = doc["bufferViews"][sp["indices"]["bufferView"]], doc["bufferViews"][sp["values"]["bufferView"]]
        idx = np.frombuffer(blob, _DT[sp["indices"]["componentType"]], sp["count"], ib["byteOffset"]).astype(np.int64)
        out[idx] = np.frombuffer(blob, dt, sp["count"] * nc, vb["byteOffset"]).reshape(-1, nc)
    if acc.get("normalized"):
        out = out / float(np.iinfo(dt).max)
    return out


def _quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _sample(times, values, interp, time, width, rotation=False):
    """glTF sampler at `time` (values: flat, `width` per key, x3 for CUBICSPLINE); None outside the keys."""
    if len(times) < 2 or time < times[0] or time > times[-1]:
        return None
    i = min(max(int(np.searchsorted(times, time, side="right")) - 1, 0), len(times) - 2)
    dt = times[i + 1] - times[i]
    u = 0.0 if dt <= 0 else (time - times[i]) / dt
    if interp == "CUBICSPLINE":
        k = values.reshape(len(times), 3, width)
        u2, u3 = u * u, u * u * u
        r = (2 * u3 - 3 * u2 + 1) * k[i, 1] + dt * (u3 - 2 * u2 + u) * k[i, 2] + (-2 * u3 + 3 * u2) * k[i + 1, 1] + dt * (u3 - u2) * k[i + 1, 0]
        return r / np.linalg.norm(r) if rotation else r
    k = values.reshape(len(times), width)
    if interp == "STEP":
        return k[i]
    a, b = k[i], k[i + 1]
    if not rotation:
        return a + (b - a) * u
    d = float(a @ b)
    if d < 0:
        b, d = -b, -d
    r = a + (b - a) * u if d > 1 - 1e-7 else (np.sin((1 - u) * np.arccos(d)) * a + np.sin(u * np.arccos(d)) * b) / np.sin(np.arccos(d))
    return r / np.linalg.norm(r)


def pose(doc, blob, clip, time):
    """(world matrix per node, weights per mesh) at `time`."""
    nodes = doc["nodes"]
    trs = [dict(t=np.array(n.get("translation", [0, 0, 0]), float), q=np.array(n.get("rotation", [0, 0, 0, 1]), float),
                s=np.array(n.get("scale", [1, 1, 1]), float)) for n in nodes]
    weights = [np.array(m.get("weights", []), float) for m in doc["meshes"]]
    anim = doc["animations"][clip]
    for ch in anim["channels"]:
        smp = anim["samplers"][ch["sampler"]]
        path, node = ch["target"]["path"], ch["target"]["node"]
        times = accessor(doc, blob, smp["input"])[:, 0]
        vals = accessor(doc, blob, smp["output"]).reshape(-1)
        interp = smp.get("interpolation", "LINEAR")
        if path == "weights":
            width = len(vals) // (len(times) * (3 if interp == "CUBICSPLINE" else 1))
            v = _sample(times, vals, interp, time, width)
            if v is not None:
                weights[nodes[node]["mesh"]] = v
            continue
        v = _sample(times, vals, interp, time, 4 if path == "rotation" else 3, path == "rotation")
        if v is not None:
            trs[node][{"translation": "t", "rotation": "q", "scale": "s"}[path]] = v
    world = [None] * len(nodes)

    def visit(n, parent):
        local = np.eye(4)
        if "matrix" in nodes[n]:
            local = np.array(nodes[n]["matrix"], float).reshape(4, 4).T
        else:
            local[:3, :3] = _quat_matrix(trs[n]["q"]) @ np.diag(trs[n]["s"])
            local[:3, 3] = trs[n]["t"]
        world[n] = parent @ local
        for c in nodes[n].get("children", []):
            visit(c, world[n])

    for r in doc["scenes"][0]["nodes"]:
        visit(r, np.eye(4))
    return world, weights


def joint_matrices(doc, blob, world, skin, ref_node):
    sk = doc["skins"][skin]
    ibm = accessor(doc, blob, sk["inverseBindMatrices"]).reshape(-1, 4, 4).transpose(0, 2, 1) if "inverseBindMatrices" in sk else np.zeros((0, 4, 4))
    inv_ref = np.linalg.inv(world[ref_node])
    return [inv_ref @ world[j] @ (ibm[i] if i < len(ibm) else np.eye(4)) for i, j in enumerate(sk["joints"])]


def arr(ptr, n, dtype=np.float32):
    """A copy of n elements behind a ctypes pointer (None for NULL)."""
    if not ptr:
        return None
    return np.ctypeslib.as_array(ptr, (n,)).astype(dtype).copy()


def deform_reference(prim, joint_table, morph_weights, dtype=np.float32):
    """The two shaders restated (shaders/morph.comp.slang then shaders/skinning.comp.slang) for one MiPtDeformPrimitive, in `dtype`.
    joint_table: (numJointMatrices, 16) column-major; returns (positions, normals or None, tangents or None)."""
    nv = prim.vertexCount
    p = arr(prim.basePositions, nv * 3).reshape(nv, 3).astype(dtype)
    n = arr(prim.baseNormals, nv * 3)
    t = arr(prim.baseTangents, nv * 4)
    n = n.reshape(nv, 3).astype(dtype) if n is not None else None
    t = t.reshape(nv, 4).astype(dtype) if t is not None else None

    def unit(v):
        return (v / np.sqrt((v * v).sum(1, keepdims=True))).astype(dtype)
    if prim.numTargets:
        nt = prim.numTargets
        dp = arr(prim.positionDeltas, nv * 3 * nt).reshape(nt, nv, 3).astype(dtype)
        dn = arr(prim.normalDeltas, nv * 3 * nt)
        dtg = arr(prim.tangentDeltas, nv * 3 * nt)
        for k in range(nt):
            w = dtype(morph_weights[prim.morphWeightOffset + k])
            if w == 0:
                continue
            p = p + w * dp[k]
            if dn is not None:
                n = n + w * dn.reshape(nt, nv, 3)[k].astype(dtype)
            if dtg is not None:
                t[:, :3] = t[:, :3] + w * dtg.reshape(nt, nv, 3)[k].astype(dtype)
        if dn is not None:
            n = unit(n)
        if dtg is not None:
            t[:, :3] = unit(t[:, :3])
    if prim.joints:
        j = arr(prim.joints, nv * 4, np.int64).reshape(nv, 4)
        w = arr(prim.weights, nv * 4).reshape(nv, 4).astype(dtype)
        J = joint_table[prim.jointMatrixOffset:prim.jointMatrixOffset + prim.numJoints].reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)
        N = np.stack([np.linalg.inv(m[:3, :3]).T for m in J]).astype(dtype) if len(J) else np.zeros((0, 3, 3), dtype)
        J = J.astype(dtype)
        sp, sn, st = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
        for i in range(4):
            ok = (w[:, i] > 0) & (j[:, i] < prim.numJoints)
            ji = np.where(ok, j[:, i], 0)
            wi = np.where(ok, w[:, i], 0).astype(dtype)[:, None]
            if not len(J):
                continue
            sp += wi * (np.einsum("vrc,vc->vr", J[ji, :3, :3], p) + J[ji, :3, 3])
            if n is not None:
                sn += wi * np.einsum("vrc,vc->vr", N[ji], n)
            if t is not None:
                st += wi * np.einsum("vrc,vc->vr", J[ji, :3, :3], t[:, :3])
        p = sp
        with np.errstate(invalid="ignore", divide="ignore"):
            if n is not None:
                n = unit(sn)
            if t is not None:
                t[:, :3] = unit(st)
    return p, n, t


def frame_tables(deform):
    return (arr(deform.jointMatrices, deform.numJointMatrices * 16).reshape(-1, 16) if deform.numJointMatrices else np.zeros((0, 16), np.float32),
            arr(deform.morphWeights, deform.numMorphWeights) if deform.numMorphWeights else np.zeros(0, np.float32))


def prims(deform):
    return [deform.prims[i] for i in range(deform.numPrims)]


def posed_desc(scene, streams):
    """A copy of scene.desc whose render primitives take `streams` ({prim: (positions, normals, tangents)} float32 arrays) instead of
    their own: the scene handed to mi_pt_create with vertices read back from another instance.  Returns (holder with .desc, keep-alive)."""
    d = scene.desc.contents
    n = d.numRenderPrimitives
    table = (type(d.renderPrimitives.contents) * n)()
    keep = []
    for i in range(n):
        C.memmove(C.byref(table[i]), C.byref(d.renderPrimitives[i]), C.sizeof(table[i]))
        if i in streams:
            for name, a in zip(("positions", "normals", "tangents"), streams[i]):
                if a is not None:
                    a = np.ascontiguousarray(a, np.float32)
                    keep.append(a)
                    setattr(table[i], name, a.ctypes.data_as(C.POINTER(C.c_float)))
    desc = type(d)()
    C.memmove(C.byref(desc), C.byref(d), C.sizeof(desc))
    desc.renderPrimitives = table

    class Holder:
        pass
    h = Holder()
    h.desc = C.pointer(desc)
    keep += [table, desc]
    return h, keep
