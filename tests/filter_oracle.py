"""Numpy checker of the instance filter (vmap_amd/instances.py, csrc/filter_kernels.h, csrc/filter_rules.h), written from the contract
of the filter section of include/vmapstep.h - one full-frame mask per id, as the reference's box_filter loops - not from the kernels.

Nothing in it can be held against Open3D or OpenCV: neither library was available where it was written.  What it pins is the
contract: float32 arithmetic with every fused multiply-add emulated exactly (a float64 product of two float32 is exact; the float64
sum is then rounded to odd, after which the rounding to float32 is the one a fused operation makes), the erosion rule, the decision
table and the label rule.  The box search is not part of it: a test hands it the device's own box table.

Frames come in as the image files hold them, [H, W]; u = column, v = row."""
from __future__ import annotations

import numpy as np

ABSENT, NEW, MERGED, UNSURE, BACKGROUND, FEW_POINTS, SMALL, MIXED, NEW_NO_BOX = range(9)
KEY_BIAS = 32768
f32 = np.float32


def fmaf(a, b, c):
    """float32(a * b + c) with one rounding, elementwise."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    s = a * b                                                   # exact: 24 + 24 bits
    with np.errstate(invalid="ignore", over="ignore"):
        t = s + c
        bb = t - s
        err = (s - (t - bb)) + (c - bb)                         # TwoSum: t + err = s + c exactly
        inexact = np.isfinite(t) & (err != 0)
        even = (np.atleast_1d(t).view(np.int64).reshape(np.shape(t)) & 1) == 0
        toward = np.nextafter(t, np.where(err > 0, np.inf, -np.inf))
        t = np.where(inexact & even, toward, t)                 # round to odd
        return t.astype(np.float32)


def depth_of(raw, depth_scale, max_depth):
    d = np.asarray(raw).astype(np.float32) * f32(depth_scale)
    with np.errstate(invalid="ignore"):
        d[d > f32(max_depth)] = 0.0
    return d


def world_points(u, v, d, intrinsics, t_wc):
    """float32 [n, 3]: t_wc . ((u - cx) / fx . d, (v - cy) / fy . d, d, 1), the fused chain innermost term first."""
    fx, fy, cx, cy = (f32(x) for x in intrinsics)
    T = np.asarray(t_wc, np.float32).reshape(4, 4)
    d = np.asarray(d, np.float32)
    xc = ((np.asarray(u).astype(np.float32) - cx) / fx) * d
    yc = ((np.asarray(v).astype(np.float32) - cy) / fy) * d
    return np.stack([fmaf(T[r, 0], xc, fmaf(T[r, 1], yc, fmaf(T[r, 2], d, T[r, 3]))) for r in range(3)], -1)


def voxel_coords(p, voxel):
    """(k int64 [n, 3], ok bool [n]): floor(p / voxel) per axis; ok where all three lie in [-32768, 32767]."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = np.floor(np.asarray(p, np.float32) / f32(voxel))
        ok = np.all((f >= -32768.0) & (f <= 32767.0), axis=-1)
    k = np.where(ok[..., None], f, 0).astype(np.int64)
    return k, ok


def pack_keys(idv, k):
    k = np.asarray(k, np.int64) + KEY_BIAS
    return (np.int64(idv) << 48) | (k[..., 0] << 32) | (k[..., 1] << 16) | k[..., 2]


def key_points(keys, voxel):
    """float32 [n, 3]: the centres of the voxels of keys."""
    keys = np.asarray(keys, np.int64)
    k = np.stack([(keys >> s) & 0xffff for s in (32, 16, 0)], -1) - KEY_BIAS
    return fmaf(k.astype(np.float32), f32(voxel), f32(0.5) * f32(voxel))


def inside_box(row, p):
    """bool [n]: |(p - centre) . axis| <= half extent on the three axes of a box-table row (float32 [16])."""
    row = np.asarray(row, np.float32)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    d = p - row[None, 0:3]
    ok = np.ones(len(p), bool)
    for a in range(3):
        ax = row[3 + 3 * a:6 + 3 * a]
        proj = fmaf(ax[0], d[:, 0], fmaf(ax[1], d[:, 1], ax[2] * d[:, 2]))
        with np.errstate(invalid="ignore"):
            ok &= np.abs(proj) <= row[12 + a]
    return ok


def erode(mask, radius, same=None):
    """The eroded mask: pixel (r, c) of ``mask`` stays iff every in-image pixel of the (2 radius + 1)^2 window around it is in the
    mask too.  Written as the definition: one shifted copy per window offset, the outside of the image counting as inside."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    padded = np.ones((H + 2 * radius, W + 2 * radius), bool)
    padded[radius:radius + H, radius:radius + W] = mask
    out = mask.copy()
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            out &= padded[dy:dy + H, dx:dx + W]
    return out


def decide(idv, pixels, c_min, c_max, valid, inside, eroded, known, min_pixels, min_points, background):
    if pixels <= 0:
        return ABSENT
    if c_min != c_max:
        return MIXED
    if c_min in [int(b) for b in background] or idv == 0:
        return BACKGROUND
    if valid <= min_points:
        return FEW_POINTS
    if known:
        return UNSURE if inside == 0 else MERGED
    return SMALL if eroded < min_pixels else NEW


def label_of(idv, status, valid, inside):
    if status == NEW:
        return idv
    if status == UNSURE:
        return -1
    if status == MERGED:
        return -1 if valid and not inside else idv
    return 0


class Filter:
    """The stateful checker.  ``put(depth, inst, sem, t_wc, box_table)`` with the box table the frame is judged against (float32
    [max_ids, 16]) returns a dict: rows int32 [n, 8] (ascending id; NEW_NO_BOX patched in), overflow, mixed (ids), out_of_grid,
    frame_keys (sorted unique int64, of the ids that stayed), labels int32 [H, W]; ``keys`` is the sorted unique state.  A NEW id
    has no box when its cloud has fewer than 4 voxels or when the caller names it in ``flat`` (flatness is the box search's call)."""

    def __init__(self, width, height, intrinsics, depth_scale, max_depth, background=(), min_pixels=1500, min_points=10, erode_radius=6,
                 voxel_size=0.01, id_shift=1, max_ids=1024):
        self.W, self.H, self.intrinsics = width, height, tuple(intrinsics)
        self.depth_scale, self.max_depth, self.background = depth_scale, max_depth, tuple(background)
        self.min_pixels, self.min_points, self.erode_radius, self.voxel, self.id_shift, self.max_ids = min_pixels, min_points, erode_radius, voxel_size, id_shift, max_ids
        self.keys = np.zeros(0, np.int64)

    def put(self, depth, inst, sem, t_wc, box_table, flat=()):
        H, W = self.H, self.W
        ids = np.asarray(inst).astype(np.int64) + self.id_shift
        sem = np.asarray(sem).astype(np.int64)
        d = depth_of(depth, self.depth_scale, self.max_depth)
        with np.errstate(invalid="ignore"):
            valid = d > 0
        v, u = np.mgrid[0:H, 0:W]
        world = world_points(u.reshape(-1), v.reshape(-1), d.reshape(-1), self.intrinsics, t_wc).reshape(H, W, 3)
        box_table = np.asarray(box_table, np.float32)
        in_range = (ids >= 0) & (ids < self.max_ids)
        out = dict(overflow=int((~in_range).sum()), mixed=[], out_of_grid=0)
        labels = np.zeros((H, W), np.int32)
        rows, frame_keys = [], []
        for i in np.unique(ids[in_range]).tolist():
            mask = ids == i
            known = bool(box_table[i, 15] != 0)
            mv = mask & valid
            inside = np.zeros((H, W), bool)
            if known:
                inside[mv] = inside_box(box_table[i], world[mv])
            er = erode(mask, self.erode_radius)
            c = sem[mask]
            st = decide(i, int(mask.sum()), int(c.min()), int(c.max()), int(mv.sum()), int(inside.sum()), int(er.sum()), known,
                        self.min_pixels, self.min_points, self.background)
            emit = er & valid if st == NEW else inside if st == MERGED else np.zeros((H, W), bool)
            k, ok = voxel_coords(world[emit], self.voxel)
            keys = np.unique(pack_keys(i, k[ok]))
            out["out_of_grid"] += int((~ok).sum())
            if st == NEW and (len(keys) < 4 or i in flat):
                st, keys = NEW_NO_BOX, keys[:0]
            if st == MIXED:
                out["mixed"].append(i)
            frame_keys.append(keys)
            rows.append([i, st, int(c.min()), int(mask.sum()), int(mv.sum()), int(inside.sum()), int(er.sum()), int((er & valid).sum())])
            labels[mask] = i if st == NEW else -1 if st == UNSURE else 0
            if st == MERGED:
                labels[mask] = i
                labels[mv & ~inside] = -1
        out["rows"] = np.asarray(rows, np.int32).reshape(-1, 8)
        out["frame_keys"] = np.unique(np.concatenate(frame_keys + [np.zeros(0, np.int64)]))
        out["labels"] = labels
        if not out["overflow"] and not out["mixed"]:
            self.keys = np.unique(np.concatenate([self.keys, out["frame_keys"]]))
        return out
