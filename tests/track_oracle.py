"""Numpy checker of the instance tracker (vmap_amd/tracking.py, csrc/track_kernels.h, csrc/track_rules.h), written from the contract
of the track section of include/vmapstep.h - one full-frame mask per detection row and one inside test per (row, candidate) pair, as
the reference's track_instance loops - not from the kernels.  Erosion, depth, world points, keys and the inside test are
tests/filter_oracle.py's.

Nothing in it can be held against Open3D or OpenCV: neither library was available where it was written.  The box search is not part
of it: a test hands it the box table the frame is judged against."""
from __future__ import annotations

import numpy as np

import filter_oracle as fo
from filter_oracle import ABSENT, BACKGROUND, FEW_POINTS, MERGED, NEW, NEW_NO_BOX, SMALL  # noqa: F401

ROW_INTS = 9


def ratio_q(match_ratio):
    return int(round(float(match_ratio) * 65536))


def matches(inside, valid, rq):
    return (int(inside) << 16) > int(rq) * int(valid)


def decide(d, cls, pixels, valid, eroded, eroded_valid, inside, min_pixels, min_points, rq, background):
    """(status, index of the matched candidate or -1); ``inside``: the counts of the row's candidates in ascending id."""
    if pixels <= 0:
        return ABSENT, -1
    if d == 0 or cls in [int(b) for b in background]:
        return BACKGROUND, -1
    if eroded <= min_pixels:
        return SMALL, -1
    if eroded_valid <= min_points:
        return FEW_POINTS, -1
    for j, n in enumerate(inside):
        if matches(n, valid, rq):
            return MERGED, j
    return NEW, -1


def label_of(idv, status, valid, inside):
    if status == NEW:
        return idv
    if status == MERGED:
        return -1 if valid and not inside else idv
    return 0


def emits(status, flags):
    return bool((status == NEW and flags & 5 == 5) or (status == MERGED and flags & 3 == 3))


class Tracker:
    """The stateful checker.  ``put(depth, det, det_classes, t_wc, box_table)`` with the box table the frame is judged against
    (float32 [max_ids, 16]) returns a dict: rows int32 [n, 9] (ascending d; NEW_NO_BOX patched in), pairs int32 [n_pairs, 3], overflow,
    unnamed (rows present without a class), full (the frame's ids would reach max_ids), out_of_grid, labels int32 [H, W], status and
    ids; ``keys`` is the sorted unique state, ``class_of`` and ``next_id`` the registry.  A NEW row has no box when its cloud has
    fewer than 4 voxels or when the caller names its id in ``flat``."""

    def __init__(self, width, height, intrinsics, depth_scale, max_depth, background=(), match_ratio=0.5, min_pixels=2000, min_points=10,
                 erode_radius=6, voxel_size=0.1, det_shift=0, max_det=256, max_ids=1024):
        self.W, self.H, self.intrinsics = width, height, tuple(intrinsics)
        self.depth_scale, self.max_depth, self.background = depth_scale, max_depth, tuple(background)
        self.rq, self.min_pixels, self.min_points, self.erode_radius, self.voxel = ratio_q(match_ratio), min_pixels, min_points, erode_radius, voxel_size
        self.det_shift, self.max_det, self.max_ids = det_shift, max_det, max_ids
        self.keys = np.zeros(0, np.int64)
        self.class_of, self.next_id = {}, 1

    def candidates(self, d, cls):
        if d == 0 or cls in self.background:
            return []
        return sorted(i for i, c in self.class_of.items() if c == cls)

    def put(self, depth, det, det_classes, t_wc, box_table, flat=()):
        H, W = self.H, self.W
        rows_img = np.asarray(det).astype(np.int64) + self.det_shift
        classes = [int(c) for c in det_classes]
        d_img = fo.depth_of(depth, self.depth_scale, self.max_depth)
        with np.errstate(invalid="ignore"):
            valid = d_img > 0
        v, u = np.mgrid[0:H, 0:W]
        world = fo.world_points(u.reshape(-1), v.reshape(-1), d_img.reshape(-1), self.intrinsics, t_wc).reshape(H, W, 3)
        box_table = np.asarray(box_table, np.float32)
        in_range = (rows_img >= 0) & (rows_img < self.max_det)
        present = np.unique(rows_img[in_range]).tolist()
        out = dict(overflow=int((~in_range).sum()), unnamed=[d for d in present if d >= len(classes)], out_of_grid=0, status={}, ids={})
        pairs = [(d, i) for d, c in enumerate(classes) for i in self.candidates(d, c)]
        counts = {}
        labels = np.zeros((H, W), np.int32)
        rows, frame_keys, new_ids, rank = [], [], {}, 0
        for d in present:
            cls = classes[d] if d < len(classes) else 0
            mask = rows_img == d
            mv = mask & valid
            er = fo.erode(mask, self.erode_radius)
            cand = self.candidates(d, cls) if d < len(classes) else []
            inside = {i: np.zeros((H, W), bool) for i in cand}
            for i in cand:
                inside[i][mv] = fo.inside_box(box_table[i], world[mv])
                counts[(d, i)] = int(inside[i].sum())
            st, j = decide(d, cls, int(mask.sum()), int(mv.sum()), int(er.sum()), int((er & valid).sum()), [counts[(d, i)] for i in cand],
                           self.min_pixels, self.min_points, self.rq, self.background)
            idv, n_in = 0, 0
            if st == NEW:
                idv, rank = self.next_id + rank, rank + 1
            elif st == MERGED:
                idv, n_in = cand[j], counts[(d, cand[j])]
            emit = er & valid if st == NEW else inside[idv] if st == MERGED else np.zeros((H, W), bool)
            k, ok = fo.voxel_coords(world[emit], self.voxel)
            keys = np.unique(fo.pack_keys(idv, k[ok]))
            out["out_of_grid"] += int((~ok).sum())
            if st == NEW and (len(keys) < 4 or idv in flat):
                st, keys = NEW_NO_BOX, keys[:0]
            if st == NEW:
                new_ids[idv] = cls
            if st in (NEW, MERGED):
                out["ids"][d] = idv
            out["status"][d] = st
            frame_keys.append(keys)
            rows.append([d, st, cls, idv, int(mask.sum()), int(mv.sum()), n_in, int(er.sum()), int((er & valid).sum())])
            if st == NEW:
                labels[mask] = idv
            elif st == MERGED:
                labels[mask] = idv
                labels[mv & ~inside[idv]] = -1
        out["rows"] = np.asarray(rows, np.int32).reshape(-1, ROW_INTS)
        out["pairs"] = np.asarray([(d, i, counts.get((d, i), 0)) for d, i in pairs], np.int32).reshape(-1, 3)
        out["frame_keys"] = np.unique(np.concatenate(frame_keys + [np.zeros(0, np.int64)]))
        out["labels"] = labels
        out["new"] = sorted(new_ids)
        out["merged"] = sorted({int(r[3]) for r in rows if r[1] == MERGED})
        out["full"] = self.next_id + rank > self.max_ids
        if not out["overflow"] and not out["unnamed"] and not out["full"]:
            self.keys = np.unique(np.concatenate([self.keys, out["frame_keys"]]))
            self.class_of.update(new_ids)
            self.next_id += rank
        return out
