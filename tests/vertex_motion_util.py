"""float64 numpy restatement of the motion of a hit on deforming geometry, written from the definition and not from
csrc/device/pt_temporal.h: the material point of a first hit is fixed by its triangle and barycentrics, so where it was in the pose before
is the barycentric interpolation of that triangle's previous-pose vertices, carried to the world by the node's previous objectToWorld:

    previous world position = prevObjectToWorld * (b0 p0 + b1 p1 + b2 p2),   b0 = 1 - b1 - b2

The current point stays the recorded first hit; projection, depth and the sky are those of temporal_util.motion_numpy.  A hit whose
triangle has previous positions equal to its current ones bit for bit, or whose record names no deforming primitive, is a rigid hit
(temporal_util.motion_numpy).  Shared by tests/test_vertex_motion_on_host.py (against the header compiled for the host) and
tests/test_gpu_vertex_motion.py (against the kernels)."""
import numpy as np

import temporal_util as tu

NO_PRIM = 0xFFFFFFFF


def barycentric_point(tri_record, prims, which):
    """Object-space points b0 v0 + b1 v1 + b2 v2 in float64 for (N, 4) uint32 triangle records; prims: {primitive id: dict(indices (T, 3),
    prev (V, 3) or None, cur (V, 3))}; which: "prev" or "cur".  Returns (points (N, 3), known (N,) bool: the record names such a primitive)."""
    tri = np.asarray(tri_record, np.uint32).reshape(-1, 4)
    b1 = np.ascontiguousarray(tri[:, 2]).view(np.float32).astype(np.float64)
    b2 = np.ascontiguousarray(tri[:, 3]).view(np.float32).astype(np.float64)
    # b0 as the hit's own float32 arithmetic leaves it: the three weights the shade interpolates with ARE float32 numbers
    b0 = (np.float32(1.0) - np.ascontiguousarray(tri[:, 2]).view(np.float32) - np.ascontiguousarray(tri[:, 3]).view(np.float32)).astype(np.float64)
    out = np.zeros((len(tri), 3))
    known = np.zeros(len(tri), bool)
    for pid, p in prims.items():
        if p.get(which) is None:
            continue
        sel = (tri[:, 0] == pid) & (tri[:, 1] < len(p["indices"]))
        if not sel.any():
            continue
        idx = np.asarray(p["indices"], np.int64)[tri[sel, 1].astype(np.int64)]
        v = np.asarray(p[which], np.float64)
        out[sel] = b0[sel, None] * v[idx[:, 0]] + b1[sel, None] * v[idx[:, 1]] + b2[sel, None] * v[idx[:, 2]]
        known |= sel
    return out, known


def triangle_moved(tri_record, prims):
    """(N,) bool: the record names a deforming primitive whose triangle's nine previous floats differ from its nine current ones in some bit."""
    tri = np.asarray(tri_record, np.uint32).reshape(-1, 4)
    moved = np.zeros(len(tri), bool)
    for pid, p in prims.items():
        if p.get("prev") is None:
            continue
        sel = (tri[:, 0] == pid) & (tri[:, 1] < len(p["indices"]))
        if not sel.any():
            continue
        idx = np.asarray(p["indices"], np.int64)[tri[sel, 1].astype(np.int64)]
        prev = np.ascontiguousarray(p["prev"], np.float32).view(np.uint32)[idx].reshape(-1, 9)
        cur = np.ascontiguousarray(p["cur"], np.float32).view(np.uint32)[idx].reshape(-1, 9)
        moved[sel] = (prev != cur).any(axis=1)
    return moved


def vertex_motion_numpy(first_hit, tri_record, prims, o2w, w2o, prev_o2w, view_proj, prev_mvp, width, height):
    """first_hit (N, 4) float32 (w = id bits), tri_record (N, 4) uint32.  Returns ((N, 3) float64: motion x, y in pixels, previous NDC
    depth; (N, 2) clip w under both cameras; (N,) bool: the hit took the deformed path)."""
    fh = np.asarray(first_hit, np.float32).reshape(-1, 4)
    out, clipw = tu.motion_numpy(fh, o2w, w2o, prev_o2w, view_proj, prev_mvp, width, height)
    ids = np.ascontiguousarray(fh[:, 3]).view(np.uint32).astype(np.int64)
    mesh = (ids != 0) & (ids != tu.ID_INVALID) & (ids <= len(o2w))
    deformed = mesh & triangle_moved(tri_record, prims)
    obj, _ = barycentric_point(tri_record, prims, "prev")
    vp, pm = tu.mat(view_proj), tu.mat(prev_mvp)
    for i in np.nonzero(deformed)[0]:
        prev_world = (tu.mat(prev_o2w[ids[i] - 1]) @ np.append(obj[i], 1.0))[:3]
        cur_clip = vp @ np.append(fh[i, :3].astype(np.float64), 1.0)
        prev_clip = pm @ np.append(prev_world, 1.0)
        out[i, :2] = (prev_clip[:2] / prev_clip[3] - cur_clip[:2] / cur_clip[3]) * 0.5 * np.array([width, height])
        out[i, 2] = prev_clip[2] / prev_clip[3]
        clipw[i] = cur_clip[3], prev_clip[3]
    return out, clipw, deformed
