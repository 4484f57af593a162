"""numpy checker of the mesh-evaluation kernels (csrc/eval_kernels.h) and of the reference's metrics (metric/metrics.py,
metric/eval_3D_obj.py:8-41), in float64: brute-force nearest neighbours, trimesh's surface-sampling formula given the uniforms,
Sutherland-Hodgman against a box's six half-spaces, and the four metrics."""
import numpy as np


def nn(queries, refs, chunk=None):
    """(distance, index) from each query to its nearest ref, float64, exhaustive; ties to the smallest index (argmin)."""
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    r = np.asarray(refs, np.float64).reshape(-1, 3)
    chunk = chunk or max(1, 2_000_000 // max(len(r), 1))
    d = np.empty(len(q))
    idx = np.empty(len(q), np.int64)
    for i in range(0, len(q), chunk):
        diff = q[i:i + chunk, None, :] - r[None, :, :]
        d2 = (diff * diff).sum(-1)
        j = d2.argmin(1)
        idx[i:i + chunk] = j
        d[i:i + chunk] = np.sqrt(d2[np.arange(len(j)), j])
    return d, idx


def runner_up_gap(queries, refs, chunk=None):
    """Second-smallest minus smallest distance per query (inf with a single ref)."""
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    r = np.asarray(refs, np.float64).reshape(-1, 3)
    chunk = chunk or max(1, 2_000_000 // max(len(r), 1))
    out = np.full(len(q), np.inf)
    if len(r) < 2:
        return out
    for i in range(0, len(q), chunk):
        d = np.sqrt(((q[i:i + chunk, None, :] - r[None, :, :]) ** 2).sum(-1))
        p = np.partition(d, 1, axis=1)
        out[i:i + chunk] = p[:, 1] - p[:, 0]
    return out


def face_areas(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)


def sample(vertices, faces, u0, r):
    """trimesh.sample.sample_surface's formula with given uniforms: face = searchsorted_left(cumsum(area), u0 * total);
    (r1, r2) -> (1 - r1, 1 - r2) if r1 + r2 > 1; point = v0 + r1 (v1 - v0) + r2 (v2 - v0).  Returns (points float64, face)."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    cdf = np.cumsum(face_areas(v, f))
    face = np.minimum(np.searchsorted(cdf, np.asarray(u0, np.float64) * cdf[-1], side="left"), len(f) - 1)
    rr = np.asarray(r, np.float64).reshape(-1, 2).copy()
    flip = rr.sum(1) > 1.0
    rr[flip] = 1.0 - rr[flip]
    v0, v1, v2 = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    return v0 + rr[:, :1] * (v1 - v0) + rr[:, 1:] * (v2 - v0), face


def clip_polygon(poly, center, R, extent):
    """Sutherland-Hodgman of one polygon ([k,3]) against h_k -+ R[:,k] . (p - c) >= 0, planes in the order (axis 0, -), (axis 0, +),
    (axis 1, -), ...; new vertices p + (s_p / (s_p - s_q)) (q - p) with p the previous vertex, q the current one."""
    P = [np.asarray(p, np.float64) for p in poly]
    c = np.asarray(center, np.float64)
    R = np.asarray(R, np.float64)
    h = np.asarray(extent, np.float64) / 2
    for pl in range(6):
        if not P:
            break
        k, sg = pl >> 1, (1.0 if pl & 1 else -1.0)
        sd = [h[k] + sg * float(R[:, k] @ (p - c)) for p in P]
        if all(s >= 0 for s in sd):
            continue
        out = []
        for i in range(len(P)):
            pv = i - 1
            if (sd[i] >= 0) != (sd[pv] >= 0):
                t = sd[pv] / (sd[pv] - sd[i])
                out.append(P[pv] + t * (P[i] - P[pv]))
            if sd[i] >= 0:
                out.append(P[i])
        P = out
    return P


def clip_mesh(vertices, faces, center, R, extent):
    """Triangle soup [T,3,3] float64: every face clipped, fan-triangulated from its first vertex, face order then fan order."""
    v = np.asarray(vertices, np.float64)
    tris = []
    for f in np.asarray(faces, np.int64):
        P = clip_polygon(v[f], center, R, extent)
        for k in range(1, len(P) - 1):
            tris.append([P[0], P[k], P[k + 1]])
    return np.asarray(tris, np.float64).reshape(-1, 3, 3)


def soup_area(tris):
    t = np.asarray(tris, np.float64)
    return float(0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum())


def accuracy(gt_points, rec_points):
    return float(nn(rec_points, gt_points)[0].mean())


def completion(gt_points, rec_points):
    return float(nn(gt_points, rec_points)[0].mean())


def completion_ratio(gt_points, rec_points, dist_th=0.01):
    return float((nn(gt_points, rec_points)[0] < dist_th).mean())


def chamfer(gt_points, rec_points):
    return (completion(gt_points, rec_points) + accuracy(gt_points, rec_points)) / 2.0


def metrics(gt_points, rec_points):
    """[[acc], [comp], [ratio_1cm], [ratio_5cm]] as eval_3D_obj.py:37-41 orders them."""
    return [[accuracy(gt_points, rec_points)], [completion(gt_points, rec_points)], [completion_ratio(gt_points, rec_points, 0.01)],
            [completion_ratio(gt_points, rec_points, 0.05)]]
