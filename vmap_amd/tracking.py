"""The instance tracker on the device: the reference's ``track_instance`` (utils.py:274-382) without Open3D or OpenCV
(csrc/track_kernels.h, csrc/track_rules.h; the contract is the track section of include/vmapstep.h).

A detector numbers its masks afresh in every frame.  Per mask the reference decides which known object it is: it erodes the mask
(``cv2.erode``), unprojects the eroded and the whole mask (Open3D), drops a small cloud, and tests the whole cloud against the box of
every known instance of the mask's class (``get_point_indices_within_bounding_box``); the first instance that holds more than
``match_ratio`` of the points takes the mask (its cloud grows, its box is refitted, points outside the old box are marked -1),
otherwise the mask founds a new instance.  ``InstanceTracker.put`` takes the frame as the image files hold it (row-major [H, W]), the
detector's label image and the class of every detection row, and keeps the state on the device in the form ``InstanceFilter`` keeps
it: a sorted voxel-key set with the persistent id above bit 48, a box table, ``boxes``, ``class_of`` and ``next_id``.  GPU only: there
is no eager path.  ``res.labels`` is in the format ``InstanceFilter.put`` returns - persistent id, 0 or -1 - and goes to
``FrameIngest.put`` in the same way.  Overlapping detector masks are resolved by the caller into one label image
(``check_mask_order`` is not part of this).

One ``put``: the host lays out the frame's pair table (per detection row the registered instances of its class, ascending - the
order of the reference's ``sem_dict[class]``) and uploads it from pinned memory; track_init, track_stats, track_decide, track_count,
track_scan, track_emit on the current stream with no host step between them; one host read of the table; from there on as the
filter: torch's ``unique`` merges the frame's keys into the sorted state, the clouds of the touched ids are decoded (voxel_points)
and their boxes searched (``bounds.oriented_bounds`` with ``min_extent``), track_write labels the frame against the boxes the
instances had when the frame arrived, and only then are the box-table rows and ``class_of`` updated.

The eroded mask, the depth rule, the world point, the voxel key and the inside test are the filter's (csrc/filter_rules.h; see
``instances.py`` for what they were and were not checked against).  Nothing in this module could be held against Open3D or OpenCV:
neither was available where it was written.  What is pinned is the contract of include/vmapstep.h.

Persistent ids start at 1 and rise in order of creation: the frame's NEW rows take ``next_id + rank`` in ascending row.  A NEW row
whose cloud has no box (fewer than 4 voxels, or flat) becomes ``NEW_NO_BOX``: label 0, not registered, its keys dropped - and its id
stays unused, so the ids of ``boxes`` can have gaps.

Deviations from the reference, all deliberate:
- all detections of a frame are judged against the boxes the instances had when the frame arrived (the reference refits a box
  after every merge, so a later mask of the same frame meets the refitted box);
- two detections of one frame are never merged with each other: two unmatched ones become two instances (the reference can merge a
  later mask into an instance an earlier mask of the same frame created);
- two detections that match the same instance both merge into it, and both keep its id in the label image (the reference keeps
  only the first in its result);
- the small-cloud test counts eroded valid points (``eroded_valid <= min_points``), not the voxels of the down-sampled eroded cloud
  (utils.py:293-295);
- as in the filter: the voxel grid is anchored at the world origin and a voxel is its centre, the box comes from
  ``bounds.oriented_bounds``' search and not from ``create_from_points``, ``box_margin`` (default 0.875 * voxel_size, for the reason
  given in ``instances.py``) is added to every half extent, and points are float32;
- classes match by equality: the CLIP-feature similarity of utils.py:305-309 is not part of this.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np
import torch

from . import _devmem, _lib, bounds
from .ingest import _device_input
from .instances import (ABSENT, BACKGROUND, FEW_POINTS, KEY_ID_SHIFT, MERGED, NEW, NEW_NO_BOX, SMALL, STATUS_NAMES, _KeyState,  # noqa: F401
                        box_row)
from .meshing import BoundingBox

__all__ = ["InstanceTracker", "TrackResult", "STATUS_NAMES", "ABSENT", "NEW", "MERGED", "BACKGROUND", "FEW_POINTS", "SMALL", "NEW_NO_BOX"]


@dataclass
class TrackResult:
    labels: torch.Tensor                   # device int32 [H, W]: persistent id, 0 or -1 per pixel
    rows: np.ndarray                       # int32 [n, 9] in ascending d: d, status, class, id, pixels, valid, inside, eroded, eroded_valid
    pairs: np.ndarray                      # int32 [n_pairs, 3]: (d, instance, inside) of every pair of the frame
    status: Dict[int, int] = field(default_factory=dict)       # every row present in the frame -> its status
    ids: Dict[int, int] = field(default_factory=dict)          # every NEW or MERGED row -> its persistent id
    new: List[int] = field(default_factory=list)               # persistent ids registered by this frame
    merged: List[int] = field(default_factory=list)            # known ids whose cloud and box this frame updated (ascending, each once)
    out_of_grid: int = 0                   # cloud points that were not inserted: a voxel coordinate outside [-32768, 32767]


class InstanceTracker(_KeyState):
    """``InstanceTracker(width, height, intrinsics, depth_scale, max_depth, ...).put(depth, det, det_classes, t_wc)``: one frame
    through ``track_instance``.  State: ``boxes`` {id: BoundingBox}, ``class_of`` {id: class}, ``next_id``, ``box_table`` (device
    float32 [max_ids, 16]), ``keys`` (sorted device int64)."""

    def __init__(self, width: int, height: int, intrinsics, depth_scale: float, max_depth: float, background_classes=(),
                 match_ratio: float = 0.5, min_pixels: int = 2000, min_points: int = 10, erode_radius: int = 6, voxel_size: float = 0.1,
                 min_extent: float = 0.05, box_margin=None, det_shift: int = 0, max_det: int = 256, max_pairs: int = 4096,
                 max_ids: int = 1024, device="cuda:0"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.VmapStepError("InstanceTracker runs on the GPU (no CPU fallback): the device must be a cuda device")
        classes = [int(c) for c in background_classes]
        if len(classes) > _lib.FILTER_MAX_CLASSES:
            raise ValueError(f"at most {_lib.FILTER_MAX_CLASSES} background classes")
        if not 1 <= int(max_det) <= _lib.TRACK_MAX_DET:
            raise ValueError(f"max_det must be in [1, {_lib.TRACK_MAX_DET}]")
        if not 1 <= int(max_pairs) <= _lib.TRACK_MAX_PAIRS:
            raise ValueError(f"max_pairs must be in [1, {_lib.TRACK_MAX_PAIRS}]")
        if not 2 <= int(max_ids) <= _lib.FILTER_MAX_IDS:
            raise ValueError(f"max_ids must be in [2, {_lib.FILTER_MAX_IDS}]")
        if not 0 <= int(erode_radius) <= _lib.FILTER_MAX_RADIUS:
            raise ValueError(f"erode_radius must be in [0, {_lib.FILTER_MAX_RADIUS}]")
        if not float(voxel_size) > 0.0:
            raise ValueError("voxel_size must be > 0")
        if not 0.0 <= float(match_ratio) <= 1.0:
            raise ValueError("match_ratio must be in [0, 1]")
        self.device, self.W, self.H = dev, int(width), int(height)
        self.intrinsics = bounds._intrinsics4(intrinsics)
        self.depth_scale, self.max_depth, self.voxel_size = float(depth_scale), float(max_depth), float(voxel_size)
        self.background_classes = tuple(classes)
        self.match_ratio, self.ratio_q = float(match_ratio), int(round(float(match_ratio) * 65536))
        self.min_pixels, self.min_points, self.erode_radius = int(min_pixels), int(min_points), int(erode_radius)
        self.min_extent = float(min_extent)
        self.box_margin = 0.875 * self.voxel_size if box_margin is None else float(box_margin)
        self.det_shift, self.max_det, self.max_pairs, self.max_ids = int(det_shift), int(max_det), int(max_pairs), int(max_ids)
        self.lib = _lib.load()
        self.next_id = 1
        cfg = self._cfg(False, False, np.eye(4), 0, 0)
        self._ws, self._ws_ptr, self._ws_bytes = _devmem.workspace(self.lib, self.lib.vmapstep_track_workspace_bytes, dev, ctypes.byref(cfg))
        n = _lib.TRACK_HEAD_INTS + self.max_det * _lib.TRACK_ROW_INTS + self.max_pairs
        self._rows_dev = torch.zeros(n, dtype=torch.int32, device=dev)
        self._rows_host = torch.zeros(n, dtype=torch.int32).pin_memory()
        n_meta = 2 * self.max_det + 1 + self.max_pairs                 # det_class, pair_off, pair_inst
        self._meta_dev = torch.zeros(n_meta, dtype=torch.int32, device=dev)
        self._meta_host = torch.zeros(n_meta, dtype=torch.int32).pin_memory()
        self._status = torch.zeros(self.max_det, dtype=torch.int32, device=dev)
        self._ident = torch.zeros(self.max_det, dtype=torch.int32, device=dev)
        self._keys_buf = torch.zeros(self.W * self.H, dtype=torch.int64, device=dev)
        self.boxes: Dict[int, BoundingBox] = {}
        self.class_of: Dict[int, int] = {}
        self._by_class: Dict[int, List[int]] = {}                      # class -> its registered ids, ascending: the candidates
        self.box_table = torch.zeros(self.max_ids, _lib.FILTER_BOX_FLOATS, dtype=torch.float32, device=dev)
        self.keys = torch.zeros(0, dtype=torch.int64, device=dev)
        self._events = {}

    def _cfg(self, depth_f32: bool, label_i32: bool, t_wc, n_det: int, n_pairs: int) -> _lib.TrackCfg:
        bg = (ctypes.c_int32 * 64)(*self.background_classes)
        pose = (ctypes.c_float * 16)(*np.asarray(t_wc, np.float32).reshape(16).tolist())
        fx, fy, cx, cy = self.intrinsics
        return _lib.TrackCfg(self.W, self.H, int(depth_f32), int(label_i32), self.depth_scale, self.max_depth, fx, fy, cx, cy, pose,
                             self.voxel_size, self.det_shift, self.min_pixels, self.min_points, self.erode_radius, self.max_det,
                             self.max_pairs, self.max_ids, n_det, n_pairs, self.next_id,
                             self.ratio_q, len(self.background_classes), bg)

    def pair_table(self, det_classes):
        """(pair_off int32 [max_det + 1], pair_inst int32 [n_pairs]) of a frame: per detection row the registered instances of its class
        in ascending id.  Row 0 and rows of a background class have none: their status does not depend on any."""
        off = np.zeros(self.max_det + 1, np.int32)
        inst: List[int] = []
        for d, c in enumerate(det_classes):
            off[d] = len(inst)
            if d != 0 and c not in self.background_classes:
                inst.extend(self._by_class.get(c, ()))
        off[len(det_classes):] = len(inst)
        return off, np.asarray(inst, np.int32)

    def put(self, depth, det, det_classes, t_wc) -> TrackResult:
        """One frame: depth u16 or f32 [H, W], det u16 or i32 [H, W] (the detector's label image; raw + det_shift = the detection row,
        row 0 = no detection), det_classes the class of every row (a host sequence), t_wc [4, 4] (camera to world).  Host tensors and
        arrays are uploaded as they are.  Raises ``ValueError`` - and leaves the state as it was - when a row of the image lies outside
        [0, max_det - 1] or has no entry in det_classes, when the frame needs more than max_pairs pairs, and when an id would reach
        max_ids."""
        dev, H, W = self.device, self.H, self.W
        self._events = {}
        classes = [int(c) for c in det_classes]
        n_det = len(classes)
        if n_det > self.max_det:
            raise ValueError(f"{n_det} detection rows, max_det = {self.max_det} (at most {_lib.TRACK_MAX_DET})")
        pair_off, pair_inst = self.pair_table(classes)
        n_pairs = int(pair_inst.size)
        if n_pairs > self.max_pairs:
            raise ValueError(f"the frame needs {n_pairs} (detection, candidate) pairs, max_pairs = {self.max_pairs} (at most {_lib.TRACK_MAX_PAIRS})")
        with torch.cuda.device(dev):
            depth, det = (_device_input(x, dev, n) for x, n in ((depth, "depth"), (det, "det")))
            if depth is None or det is None:
                raise TypeError("InstanceTracker.put: depth and det are required")
            if depth.dtype not in (torch.uint16, torch.float32) or tuple(depth.shape) != (H, W):
                raise ValueError(f"depth must be uint16 or float32 [{H}, {W}], got {depth.dtype} {tuple(depth.shape)}")
            if det.dtype not in (torch.uint16, torch.int32) or tuple(det.shape) != (H, W):
                raise ValueError(f"det must be uint16 or int32 [{H}, {W}], got {det.dtype} {tuple(det.shape)}")
            pose = (t_wc.detach().cpu().numpy() if torch.is_tensor(t_wc) else np.asarray(t_wc)).astype(np.float32).reshape(4, 4)
            cfg = self._cfg(depth.dtype == torch.float32, det.dtype == torch.int32, pose, n_det, n_pairs)
            stream = _devmem.stream(dev)

            # the frame's pair table: one pinned upload, nothing waits (the last put's read has synchronised since the last upload)
            meta = self._meta_host.numpy()
            meta[:self.max_det] = 0
            meta[:n_det] = classes
            meta[self.max_det:2 * self.max_det + 1] = pair_off
            meta[2 * self.max_det + 1:2 * self.max_det + 1 + n_pairs] = pair_inst
            n_meta = 2 * self.max_det + 1 + n_pairs
            self._meta_dev[:n_meta].copy_(self._meta_host[:n_meta], non_blocking=True)

            self._mark("kernels")
            _lib.check(self.lib.vmapstep_track_stats(ctypes.byref(cfg), depth.data_ptr(), det.data_ptr(), self._meta_dev.data_ptr(),
                                                     self.box_table.data_ptr(), self._status.data_ptr(), self._ident.data_ptr(),
                                                     self._rows_dev.data_ptr(), self._ws_ptr, self._ws_bytes, stream), self.lib)
            _lib.check(self.lib.vmapstep_track_emit(ctypes.byref(cfg), depth.data_ptr(), det.data_ptr(), self.box_table.data_ptr(),
                                                    self._status.data_ptr(), self._ident.data_ptr(), self._keys_buf.data_ptr(),
                                                    self._rows_dev.data_ptr(), self._ws_ptr, self._ws_bytes, stream), self.lib)
            self._mark("kernels")
            self._mark("read")
            self._rows_host.copy_(self._rows_dev, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            self._mark("read")
            head = self._rows_host.numpy()
            n_rows, overflow, n_keys, out_of_grid = (int(x) for x in head[:_lib.TRACK_HEAD_INTS])
            if overflow:
                raise ValueError(f"{overflow} pixels carry detection rows outside [0, {self.max_det - 1}] (raw + det_shift): "
                                 f"raise max_det (at most {_lib.TRACK_MAX_DET})")
            rows = head[_lib.TRACK_HEAD_INTS:_lib.TRACK_HEAD_INTS + n_rows * _lib.TRACK_ROW_INTS].reshape(n_rows, _lib.TRACK_ROW_INTS).copy()
            unnamed = rows[rows[:, 0] >= n_det, 0]
            if unnamed.size:
                raise ValueError(f"detection row {int(unnamed[0])} is present in the image but has no entry in det_classes ({n_det} entries)")
            n_new = int((rows[:, 1] == NEW).sum())
            if self.next_id + n_new > self.max_ids:
                raise ValueError(f"{n_new} new instances from id {self.next_id} on would reach max_ids = {self.max_ids} (at most {_lib.FILTER_MAX_IDS})")
            p0 = _lib.TRACK_HEAD_INTS + self.max_det * _lib.TRACK_ROW_INTS
            pair_d = np.repeat(np.arange(self.max_det, dtype=np.int32), np.diff(pair_off))
            pairs = np.stack([pair_d, pair_inst, head[p0:p0 + n_pairs]], 1).astype(np.int32).reshape(n_pairs, 3)
            touched = sorted({int(r[3]) for r in rows if r[1] in (NEW, MERGED)})

            # the frame's keys into the sorted unique state, and the segments of the touched ids in it
            self._mark("sort_merge")
            keys = torch.unique(torch.cat([self.keys, self._keys_buf[:n_keys]]))
            seg = np.zeros((2, 0), np.int64)
            if touched:
                ids_t = torch.tensor(touched, dtype=torch.int64, device=dev)
                seg = torch.stack([torch.searchsorted(keys, ids_t << KEY_ID_SHIFT), torch.searchsorted(keys, (ids_t + 1) << KEY_ID_SHIFT)]).cpu().numpy()
            self._mark("sort_merge")

            # the clouds of the touched ids and their boxes
            self._mark("search")
            found: Dict[int, BoundingBox] = {}
            with_keys = [k for k in range(len(touched)) if seg[1, k] > seg[0, k]]
            if with_keys:
                offsets = np.concatenate([[0], np.cumsum([seg[1, k] - seg[0, k] for k in with_keys])]).astype(np.int64)
                sel = torch.cat([keys[seg[0, k]:seg[1, k]] for k in with_keys])
                points, bnd = self._decode(sel, offsets)
                boxes = bounds.oriented_bounds(points, offsets, backend="hip", bounds=bnd, min_extent=self.min_extent)
                found = {touched[k]: b for k, b in zip(with_keys, boxes) if b is not None}
            self._mark("search")

            res = TrackResult(torch.empty(H, W, dtype=torch.int32, device=dev), rows, pairs, out_of_grid=out_of_grid)
            no_box_rows, no_box_ids, new_class = [], [], {}
            for r in rows:
                d, s, i = int(r[0]), int(r[1]), int(r[3])
                if s == MERGED:
                    assert i in found, f"id {i}: a merged cloud contains one that had a box"
                    res.ids[d] = i
                    if i not in res.merged:
                        res.merged.append(i)
                elif s == NEW and i in found:
                    res.ids[d] = i
                    res.new.append(i)
                    new_class[i] = int(r[2])
                elif s == NEW:
                    r[1] = s = NEW_NO_BOX
                    no_box_rows.append(d)
                    no_box_ids.append(i)
                res.status[d] = s
            res.merged.sort()
            if no_box_rows:
                self._status.index_fill_(0, torch.tensor(no_box_rows, dtype=torch.int64, device=dev), NEW_NO_BOX)
                keys = keys[~torch.isin(keys >> KEY_ID_SHIFT, torch.tensor(no_box_ids, dtype=torch.int64, device=dev))]

            # the labels against the boxes the instances had when the frame arrived; only then the new boxes
            self._mark("write")
            _lib.check(self.lib.vmapstep_track_write(ctypes.byref(cfg), depth.data_ptr(), det.data_ptr(), self.box_table.data_ptr(),
                                                     self._status.data_ptr(), self._ident.data_ptr(), res.labels.data_ptr(), stream), self.lib)
            if found:
                ids = sorted(found)
                table = np.stack([box_row(found[i], self.box_margin) for i in ids])
                self.box_table[torch.tensor(ids, dtype=torch.int64, device=dev)] = torch.from_numpy(table).to(dev)
            self._mark("write")
        self.keys = keys
        self.boxes.update(found)
        for i in sorted(new_class):
            self.class_of[i] = new_class[i]
            self._by_class.setdefault(new_class[i], []).append(i)
        self.next_id += n_new
        return res
