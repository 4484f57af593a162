"""Numpy checker of visibility culling (vmap_amd/visibility.py, csrc/cull_kernels.h, csrc/cull_rules.h), written from the contract of
the cull section of include/vmapstep.h, not from the kernels.  Nothing in it can be held against an outside implementation: the
contract is this project's own.  Two layers:

- ``seen_f32``: the float32 arithmetic of the contract with every fused multiply-add emulated exactly (filter_oracle.fmaf); the host
  program and the device must equal it bit for bit;
- ``seen_f64``: the geometry in float64, with the distance of every decision from its boundary, so that a test can say which points
  the float32 result may legitimately differ on (``ambiguous``) and hold every other point to the geometry.

Depth images are [K, W, H], width-major; poses [K, 4, 4] camera to world."""
from __future__ import annotations

import numpy as np

from filter_oracle import fmaf

f32 = np.float32

# The bands of ``seen_f64``.  A float32 evaluation of u = fx * c0 / z + cx carries a few roundings of relative size 2^-24 on values up
# to the image width (tests: <= 64 pixels, coordinates <= 8 m): |error| < 64 * 6 * 2^-24 + ulp(64) / 2 < 3e-5 pixel, and of z a few
# ulp of 8 m: < 3e-6 m.  The bands leave a factor of three.
PIXEL_BAND = 1e-4
DEPTH_BAND = 1e-5


def seen_by_frame_f32(points, T, intrinsics, width, height, depth=None, eps=None, margin=0, min_depth=0.0):
    """bool [n]: the contract's rule for one frame.  T: the pose (any shape holding 16 or 12 floats, row-major); depth [W, H] is read
    only where eps is not None."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float32).reshape(-1)
    fx, fy, cx, cy = (f32(x) for x in intrinsics)
    with np.errstate(all="ignore"):
        q0, q1, q2 = p[:, 0] - T[3], p[:, 1] - T[7], p[:, 2] - T[11]
        c = [fmaf(T[8 + i], q2, fmaf(T[4 + i], q1, T[i] * q0)) for i in range(3)]
        z = c[2]
        ok = z > f32(min_depth)
        u = fmaf(fx, c[0] / z, cx)
        v = fmaf(fy, c[1] / z, cy)
        w, h = np.rint(u), np.rint(v)                      # half to even
        ok &= (w >= f32(margin)) & (w <= f32(width - 1 - margin)) & (h >= f32(margin)) & (h <= f32(height - 1 - margin))
        if eps is not None:
            wi = np.where(ok, w, 0).astype(np.int64)
            hi = np.where(ok, h, 0).astype(np.int64)
            d = np.asarray(depth, np.float32)[wi, hi]
            ok &= (d > 0) & (z <= d + f32(eps))
    return ok


def seen_f32(points, depth, t_wc, intrinsics, width, height, eps=None, margin=0, min_depth=0.0, slots=None, seen=None):
    """uint8 [n]: seen by any frame.  ``slots``: frame k reads slot slots[k]; ``seen``: the mask to add to."""
    t_wc = np.asarray(t_wc, np.float32).reshape(-1, 4, 4)
    slots = range(len(t_wc)) if slots is None else [int(s) for s in slots]
    n = len(np.asarray(points).reshape(-1, 3))
    out = np.zeros(n, bool) if seen is None else np.asarray(seen).astype(bool).copy()
    for s in slots:
        out |= seen_by_frame_f32(points, t_wc[s], intrinsics, width, height, None if eps is None else depth[s], eps, margin, min_depth)
    return out.astype(np.uint8)


def seen_f64(points, depth, t_wc, intrinsics, width, height, eps=None, margin=0, min_depth=0.0, slots=None):
    """(seen bool [n], ambiguous bool [n]) in float64: c = R^T (p - t), u = fx c0 / z + cx, the nearest pixel, the comparisons.
    A point is ambiguous when, in some frame, a decision that is reached lies within its band of the boundary: z = min_depth
    (DEPTH_BAND), a projection within PIXEL_BAND of x.5 - a rounding tie, which is also where the image edge lies - or
    z = d + eps (DEPTH_BAND).  A NaN point is never seen and never ambiguous; an all-zero rotation sees nothing."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    t_wc = np.asarray(t_wc, np.float64).reshape(-1, 4, 4)
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    slots = range(len(t_wc)) if slots is None else [int(s) for s in slots]
    seen, amb = np.zeros(len(p), bool), np.zeros(len(p), bool)
    finite = np.isfinite(p).all(1)
    for s in slots:
        R, t = t_wc[s, :3, :3], t_wc[s, :3, 3]
        if not R.any():                                    # an unused slot: z is exactly 0 in any precision - nothing seen, nothing in doubt
            continue
        with np.errstate(all="ignore"):
            c = (np.where(finite[:, None], p, 0.0) - t) @ R            # rows: R^T (p - t)
            z = c[:, 2]
            front = z > min_depth
            a = np.abs(z - min_depth) <= DEPTH_BAND
            u, v = fx * c[:, 0] / z + cx, fy * c[:, 1] / z + cy
            w, h = np.rint(u), np.rint(v)
            inside = (w >= margin) & (w <= width - 1 - margin) & (h >= margin) & (h <= height - 1 - margin)
            tie = (np.abs(np.abs(u - np.floor(u)) - 0.5) <= PIXEL_BAND) | (np.abs(np.abs(v - np.floor(v)) - 0.5) <= PIXEL_BAND)
            near_image = (u > margin - 1) & (u < width - margin) & (v > margin - 1) & (v < height - margin)
            a |= front & tie & near_image
            ok = front & inside
            if eps is not None:
                wi, hi = np.where(ok, w, 0).astype(np.int64), np.where(ok, h, 0).astype(np.int64)
                d = np.asarray(depth[s], np.float64)[wi, hi]
                a |= ok & (d > 0) & (np.abs(z - (d + eps)) <= DEPTH_BAND)
                ok &= (d > 0) & (z <= d + eps)
        seen |= ok & finite
        amb |= a & finite
    return seen, amb


def cull_faces(faces, seen, min_seen):
    """(faces_out int32 [f, 3], kept_vertices int32 [v]): plain numpy.  A face is kept iff at least min_seen corners are seen; the
    kept vertices are those a kept face references, ascending; faces keep their order."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    seen = np.asarray(seen) != 0
    keep = seen[faces].sum(1) >= min_seen
    kf = faces[keep]
    kept_vertices = np.unique(kf)
    new = np.full(len(seen), -1, np.int64)
    new[kept_vertices] = np.arange(len(kept_vertices))
    return new[kf].astype(np.int32).reshape(-1, 3), kept_vertices.astype(np.int32)
