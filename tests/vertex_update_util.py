"""Shared by the vertex-update tests (mi_pt_set_vertex_updates / mi_pt_update_vertices): the interleaving loop of mi_pt_create and the normal
rebuild restated in numpy from their definitions, the vertex-to-incident-corner table, and the poses the tests drive scene_dynamic with."""
import numpy as np

NORMAL_BOUND = 2e-6  # absolute, on unit normals: the figure tests/test_gpu_deform.py uses for normals


def interleave(positions, normals=None, uv0=None, tangents=None):
    """DevPrim::verts as mi_pt_create uploads it: (V, 12) float32 = {p.xyz, n.x} {n.y, n.z, uv0} {tangent}, absent attributes zero."""
    nv = len(positions)
    out = np.zeros((nv, 12), np.float32)
    out[:, 0:3] = positions
    if normals is not None:
        out[:, 3:6] = normals
    if uv0 is not None:
        out[:, 6:8] = uv0
    if tangents is not None:
        out[:, 8:12] = tangents
    return out


def corner_table(indices, num_vertices):
    """(cornerEnd (V,), corners (3 T,)) uint32: per vertex the end of its run of incident corners (3 * triangle + corner), runs ascending."""
    flat = np.asarray(indices, np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")  # (stable: ascending corner id inside a vertex's run)
    counts = np.bincount(flat, minlength=num_vertices)
    return np.cumsum(counts).astype(np.uint32), order.astype(np.uint32)


def rebuilt_normals_f64(positions, indices, resident):
    """The normal rebuild from its definition, in float64 on the float32 positions: per vertex the sum of cross(p1 - p0, p2 - p0) over
    its incident corners, divided by its length; a vertex whose sum has no length keeps `resident`.  Returns (normals, kept mask)."""
    p = np.asarray(positions, np.float64)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    face = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]])
    s = np.zeros_like(p)
    for k in range(3):
        np.add.at(s, idx[:, k], face)
    ln = np.sqrt((s * s).sum(1))
    kept = ~(ln > 0)
    out = np.where(kept[:, None], np.asarray(resident, np.float64), s / np.where(kept, 1.0, ln)[:, None])
    return out, kept


# ---- poses of scene_dynamic ------------------------------------------------------------------------------------------------------------
def cloth_wave(rest, phase, amplitude=0.12):
    """A travelling wave on the cloth (a z-facing grid): z = A sin(5 x + phase) cos(3 y).  Returns (positions, unit normals, tangents
    (x derivative, w = 1)) in float32, the normals and tangents analytic."""
    x, y = rest[:, 0].astype(np.float64), rest[:, 1].astype(np.float64)
    z = amplitude * np.sin(5 * x + phase) * np.cos(3 * y)
    dzdx = amplitude * 5 * np.cos(5 * x + phase) * np.cos(3 * y)
    dzdy = -amplitude * 3 * np.sin(5 * x + phase) * np.sin(3 * y)
    pos = np.stack([x, y, rest[:, 2] + z], 1)
    nrm = np.stack([-dzdx, -dzdy, np.ones_like(x)], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tan = np.stack([np.ones_like(x), np.zeros_like(x), dzdx], 1)
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    return pos.astype(np.float32), nrm.astype(np.float32), np.concatenate([tan, np.ones((len(x), 1))], 1).astype(np.float32)


def ball_pulse(rest, rest_normals, phase, amplitude=0.25):
    """A radial pulse: every vertex moves along its (radial) normal by A sin(4 theta + phase) of the radius.  Normals are supplied as the
    rest ones (a shading choice of the caller: the test only needs them to arrive)."""
    r = np.linalg.norm(rest.astype(np.float64), axis=1, keepdims=True)
    d = rest / np.maximum(r, 1e-12)
    scale = 1.0 + amplitude * np.sin(4 * np.arccos(np.clip(d[:, 1:2], -1, 1)) + phase)
    return (rest * scale).astype(np.float32), np.asarray(rest_normals, np.float32).copy()


def box_shear(rest, amount):
    out = rest.astype(np.float64).copy()
    out[:, 0] += amount * out[:, 1]
    return out.astype(np.float32)


def triangle_move(rest, offset):
    return (rest.astype(np.float64) + np.asarray(offset, np.float64)).astype(np.float32)
