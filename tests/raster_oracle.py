"""Numpy checker of the mesh rasteriser (vmap_amd/raster.py, csrc/raster_kernels.h, csrc/raster_rules.h), written from the contract of
the raster section of include/vmapstep.h, not from the kernels.  Nothing in it can be held against an outside implementation: the
contract is this project's own.  Two layers:

- ``raster_f32``: the exact emulation - the float32 projection with every fused multiply-add emulated exactly (filter_oracle.fmaf),
  integers for snapping and coverage (int64: every product stays below 2^47, so they are as exact as Python's own), float64 with
  every operation rounded on its own for the depth.  The host program and the device must equal it bit for bit;
- ``raster_f64``: the geometry in float64 - ``pixel_ray`` against the unsnapped triangles, the nearest hit wins - with, per pixel,
  whether its centre lies within ``BAND`` pixels of any projected edge (such a pixel is ambiguous: snapping may move an edge across
  it) and the gradient of the winning face's reciprocal depth, from which a test derives how far snapping may move the depth.

Images are [K, W, H], width-major; poses [K, 4, 4] camera to world; pixel (w, h) has its centre at u = w, v = h."""
from __future__ import annotations

import numpy as np

from filter_oracle import fmaf

f32 = np.float32
GUARD = 16384.0
BAND = 1.0 / 64
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def snap_vertices(vertices, T, intrinsics, min_depth):
    """(X int64 [n], Y int64 [n], z float32 [n], ok bool [n]) of one view: the contract's corner rule."""
    p = np.asarray(vertices, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float32).reshape(-1)
    fx, fy, cx, cy = (f32(x) for x in intrinsics)
    with np.errstate(all="ignore"):
        q0, q1, q2 = p[:, 0] - T[3], p[:, 1] - T[7], p[:, 2] - T[11]
        c = [fmaf(T[8 + i], q2, fmaf(T[4 + i], q1, T[i] * q0)) for i in range(3)]
        z = c[2]
        ok = z > f32(min_depth)
        u = fmaf(fx, c[0] / z, cx)
        v = fmaf(fy, c[1] / z, cy)
        ok &= (np.abs(u) <= f32(GUARD)) & (np.abs(v) <= f32(GUARD))
        X = np.rint(np.where(ok, u, 0) * f32(256.0)).astype(np.int64)          # half to even; the product is exact
        Y = np.rint(np.where(ok, v, 0) * f32(256.0)).astype(np.int64)
    return X, Y, z, ok


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def raster_f32(vertices, faces, t_wc, intrinsics, width, height, min_depth, max_depth=None, slots=None):
    """dict(depth float32 [K, W, H], face int32 [K, W, H], dropped int64 [K], covered int32 [K, W, H]): ``covered`` counts the faces
    whose coverage rule holds at the pixel's centre, before any depth cut."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    t_wc = np.asarray(t_wc, np.float32).reshape(-1, 4, 4)
    slots = list(range(len(t_wc))) if slots is None else [int(s) for s in slots]
    K, nv = len(slots), len(vertices)
    depth = np.zeros((K, width, height), np.float32)
    face_img = np.full((K, width, height), -1, np.int32)
    covered = np.zeros((K, width, height), np.int32)
    dropped = np.zeros(K, np.int64)
    in_range = ((faces >= 0) & (faces < nv)).all(1)
    safe = np.where(in_range[:, None], faces, 0)
    for k, s in enumerate(slots):
        X, Y, z, ok = snap_vertices(vertices, t_wc[s], intrinsics, min_depth)
        part = in_range & ok[safe].all(1) if nv else np.zeros(len(faces), bool)
        dropped[k] = int((~part).sum())
        keys = np.full((width, height), EMPTY, np.uint64)
        A_all = _edge(X[safe[:, 0]], Y[safe[:, 0]], X[safe[:, 1]], Y[safe[:, 1]], X[safe[:, 2]], Y[safe[:, 2]]) if nv else np.zeros(len(faces), np.int64)
        for f in np.nonzero(part & (A_all != 0))[0]:                 # a zero-area face covers nothing (the loop below says so again)
            i0, i1, i2 = (int(i) for i in faces[f])
            xs, ys, zs = [int(X[i0]), int(X[i1]), int(X[i2])], [int(Y[i0]), int(Y[i1]), int(Y[i2])], [z[i0], z[i1], z[i2]]
            A = _edge(xs[0], ys[0], xs[1], ys[1], xs[2], ys[2])
            if A == 0:
                continue
            if A < 0:                                            # corners 1 and 2 change places, their depths with them
                xs[1], xs[2], ys[1], ys[2], zs[1], zs[2] = xs[2], xs[1], ys[2], ys[1], zs[2], zs[1]
                A = -A
            w0, w1 = max(-(-min(xs) // 256), 0), min(max(xs) // 256, width - 1)
            h0, h1 = max(-(-min(ys) // 256), 0), min(max(ys) // 256, height - 1)
            if w0 > w1 or h0 > h1:
                continue
            px = (np.arange(w0, w1 + 1, dtype=np.int64) * 256)[:, None]
            py = (np.arange(h0, h1 + 1, dtype=np.int64) * 256)[None, :]
            inside = np.ones((w1 - w0 + 1, h1 - h0 + 1), bool)
            E = []
            for i in range(3):
                a, b = (i + 1) % 3, (i + 2) % 3
                e = _edge(xs[a], ys[a], xs[b], ys[b], px, py)
                dx, dy = xs[b] - xs[a], ys[b] - ys[a]
                owns = dy > 0 or (dy == 0 and dx > 0)
                inside &= (e > 0) | ((e == 0) & owns)
                E.append(e)
            if not inside.any():
                continue
            covered[k, w0:w1 + 1, h0:h1 + 1] += inside
            with np.errstate(all="ignore"):
                Ad = np.float64(A)
                inv = [np.float64(1.0) / np.float64(zz) for zz in zs]
                lam = [e.astype(np.float64) / Ad for e in E]
                r = (lam[0] * inv[0] + lam[1] * inv[1]) + lam[2] * inv[2]
                zf = (np.float64(1.0) / r).astype(np.float32)
                write = inside & np.isfinite(zf) & (zf > f32(min_depth))
                if max_depth is not None and max_depth > 0:
                    write &= ~(zf > f32(max_depth))
            key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            sub = keys[w0:w1 + 1, h0:h1 + 1]
            keys[w0:w1 + 1, h0:h1 + 1] = np.where(write & (key < sub), key, sub)
        hit = keys != EMPTY
        depth[k] = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), f32(0))
        face_img[k] = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return dict(depth=depth, face=face_img, dropped=dropped, covered=covered)


def visible_faces(face_img, n_faces):
    """uint8 [n_faces]: the faces that won at least one pixel of a face image stack."""
    seen = np.zeros(n_faces, np.uint8)
    won = np.unique(face_img[face_img >= 0])
    seen[won] = 1
    return seen


def raster_f64(vertices, faces, T, intrinsics, width, height, min_depth):
    """One view in float64: dict(hit bool [W, H], depth [W, H], face [W, H], ambiguous bool [W, H], g_u [W, H], g_v [W, H]).  A face
    takes part iff its indices are in range and every corner has z > min_depth inside the guard band; the ray of pixel (w, h) is
    ((w - cx) / fx, (h - cy) / fy, 1) in the camera frame, so the ray parameter is the depth.  With M = the camera-space corners as
    columns, mu = M^-1 d: the hit is inside iff every mu_i > 0, its reciprocal depth is sum(mu) - affine in (u, v), whence the
    gradient.  A face whose M is singular (zero area, or seen edge-on through the camera centre) is never hit, but its edges count for
    ``ambiguous`` like everyone's."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(4, 4)
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    R, t = T[:3, :3], T[:3, 3]
    with np.errstate(all="ignore"):
        c = (v - t) @ R
        u, vv = fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy
        okv = (c[:, 2] > min_depth) & (np.abs(u) <= GUARD) & (np.abs(vv) <= GUARD)
    in_range = ((faces >= 0) & (faces < len(v))).all(1)
    w, h = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64), indexing="ij")
    d = np.stack([(w - cx) / fx, (h - cy) / fy, np.ones_like(w)], -1)          # [W, H, 3]
    best = np.full((width, height), np.inf)
    face_img = np.full((width, height), -1, np.int64)
    g_u, g_v = np.zeros((width, height)), np.zeros((width, height))
    amb = np.zeros((width, height), bool)
    for f in np.nonzero(in_range)[0]:
        idx = faces[f]
        if not okv[idx].all():
            continue
        for a, b in ((0, 1), (1, 2), (2, 0)):                                  # the distance of every centre from the projected edge
            ax, ay, bx, by = u[idx[a]], vv[idx[a]], u[idx[b]], vv[idx[b]]
            ex, ey = bx - ax, by - ay
            ll = ex * ex + ey * ey
            s = np.clip(((w - ax) * ex + (h - ay) * ey) / ll, 0.0, 1.0) if ll > 0 else np.zeros_like(w)
            amb |= np.hypot(w - (ax + s * ex), h - (ay + s * ey)) <= BAND
        M = c[idx].T                                                           # columns: the corners
        if abs(np.linalg.det(M)) < 1e-14:
            continue
        Mi = np.linalg.inv(M)
        mu = d @ Mi.T                                                          # [W, H, 3]
        r = mu.sum(-1)
        with np.errstate(all="ignore"):
            zz = 1.0 / r
        inside = (mu > 0).all(-1) & (zz > min_depth) & (zz < best)
        best = np.where(inside, zz, best)
        face_img = np.where(inside, f, face_img)
        g_u = np.where(inside, Mi[:, 0].sum() / fx, g_u)
        g_v = np.where(inside, Mi[:, 1].sum() / fy, g_v)
    hit = np.isfinite(best)
    return dict(hit=hit, depth=np.where(hit, best, 0.0), face=face_img, ambiguous=amb, g_u=g_u, g_v=g_v)


def compare_counts(a, b):
    """int64 [K, 4] = {n_both, n_a_only, n_b_only, sum_q} per view, by the contract's integer rule."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    K = a.shape[0]
    a, b = a.reshape(K, -1), b.reshape(K, -1)
    with np.errstate(all="ignore"):
        ma, mb = a > 0, b > 0
        both = ma & mb
        dd = np.abs(a - b)                                                     # one rounded float32 subtraction
        q = np.rint(np.where(np.isfinite(dd), dd, 0).astype(np.float64) * 2.0 ** 20)
        q = np.minimum(q, 2.0 ** 40).astype(np.int64)
    out = np.zeros((K, 4), np.int64)
    out[:, 0], out[:, 1], out[:, 2] = both.sum(1), (ma & ~mb).sum(1), (~ma & mb).sum(1)
    out[:, 3] = np.where(both, q, 0).sum(1)
    return out


def l1_of(counts):
    """metres per view: sum_q / 2^20 / n_both, NaN where n_both == 0."""
    counts = np.asarray(counts, np.int64)
    with np.errstate(all="ignore"):
        return np.where(counts[:, 0] > 0, counts[:, 3] / 2.0 ** 20 / np.maximum(counts[:, 0], 1), np.nan)
