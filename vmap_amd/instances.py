"""The instance filter on the device: ScanNet's ``box_filter`` (utils.py:112-208, called by ``ScanNet.__getitem__``, dataset.py:249-264)
without Open3D or OpenCV (csrc/filter_kernels.h, csrc/filter_rules.h; the contract is the filter section of include/vmapstep.h).

Per frame the reference decides what becomes of every instance id: kept as a new object, merged into the object already known under
that id (its cloud grows, its 3-D box is refitted), marked "unsure" (-1), or dropped to background (0).  It does so on the host with
one full-frame pass per instance: ``cv2.erode``, Open3D's unprojection, ``voxel_down_sample``, ``OrientedBoundingBox.create_from_points``
and ``get_point_indices_within_bounding_box``.  ``InstanceFilter.put`` takes the frame as the image files hold it (row-major [H, W],
after the caller's resize and edge crop) and keeps the state - a voxel-key set and a box table - on the device.  GPU only: there is
no eager path.  ``res.labels`` is what ``box_filter`` returns; it goes to ``FrameIngest.put(rgb, depth, res.labels, None, t_wc,
frame_id)`` on a ``FrameIngest`` built with ``background_classes=()``, ``min_box=-1``.  Reading files, resize and crop stay with the caller; the reference's
``track_instance`` is ``tracking.InstanceTracker``.

One ``put``: filter_init, filter_stats, filter_decide, filter_count, filter_scan, filter_emit on the current stream with no host step
between them, one host read of the table; torch's ``unique`` merges the frame's keys into the sorted state (the id is in a key's high
bits, so the state is segmented by id); the clouds of the touched ids are decoded (voxel_points) and their boxes searched
(``bounds.oriented_bounds``); filter_write labels the frame against the boxes the ids had when the frame arrived, and only then are
the box-table rows of the touched ids rewritten - as the reference uses a box before it refits it.

The eroded mask: a pixel is in it iff every in-image pixel of the (2 * erode_radius + 1)^2 window around it carries the same id.
The reference's three iterations of a 5 x 5 ``cv2.erode`` with the default border are taken to be this rule at radius 6; it was checked
against ``scipy.ndimage.binary_erosion(mask, ones((5, 5)), iterations=3, border_value=1)``, not against OpenCV, which was not at hand.

The inside test is ``|(p - centre) . axis| <= half extent`` on all three axes; ``<=`` is what Open3D's
``get_point_indices_within_bounding_box`` is believed to use - Open3D was not available where this was written, so that could not be
checked.

Deviations from the reference, all deliberate:
- the voxel grid is anchored at the world origin and a voxel is represented by its centre (Open3D anchors the grid at each cloud's
  minimum and keeps the mean of a voxel's points): the cloud is a set, so the result does not depend on the order of arrival;
- the box comes from ``bounds.oriented_bounds``' search over orientations, not from Open3D's ``create_from_points``;
- ``box_margin`` (default 0.875 * voxel_size) is added to every half extent: a raw point lies up to half a voxel diagonal
  (0.866 * voxel_size) from the centre that stands for it, so a box fitted to centres alone would reject points it was fitted to;
  with the margin every point that was merged is inside the next box.  The reference, with ``bbox3d_scale = 1.0``, marks such
  points -1;
- points are float32 (Open3D works in float64);
- a NEW id whose cloud has no box (fewer than 4 voxels, or flat) becomes ``NEW_NO_BOX``: label 0, not registered, its keys dropped
  - the reference's ``RuntimeError`` branch.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np
import torch

from . import _devmem, _lib, bounds
from .ingest import SCANNET_BACKGROUND_CLASSES, _device_input
from .meshing import BoundingBox

__all__ = ["InstanceFilter", "FilterResult", "STATUS_NAMES", "ABSENT", "NEW", "MERGED", "UNSURE", "BACKGROUND", "FEW_POINTS", "SMALL",
           "MIXED", "NEW_NO_BOX"]

ABSENT, NEW, MERGED, UNSURE, BACKGROUND, FEW_POINTS, SMALL, MIXED, NEW_NO_BOX = range(9)
STATUS_NAMES = ("ABSENT", "NEW", "MERGED", "UNSURE", "BACKGROUND", "FEW_POINTS", "SMALL", "MIXED", "NEW_NO_BOX")
KEY_ID_SHIFT = 48


@dataclass
class FilterResult:
    labels: torch.Tensor                   # device int32 [H, W]: id, 0 or -1 per pixel - what box_filter returns
    rows: np.ndarray                       # int32 [n, 8] in ascending id: id, status, class, pixels, valid, inside, eroded, eroded_valid
    status: Dict[int, int] = field(default_factory=dict)       # every id present in the frame -> its status
    counts: Dict[int, int] = field(default_factory=dict)       # every id present -> its pixels
    classes: Dict[int, int] = field(default_factory=dict)      # every id present -> its class
    new: List[int] = field(default_factory=list)               # registered by this frame
    merged: List[int] = field(default_factory=list)            # known ids whose cloud and box this frame updated
    out_of_grid: int = 0                   # cloud points that were not inserted: a voxel coordinate outside [-32768, 32767]


def box_row(box: BoundingBox, margin: float) -> np.ndarray:
    """The box-table row of a ``BoundingBox``: centre, the three axes (the columns of R), 0.5 * extent + margin, known = 1; float32."""
    row = np.zeros(_lib.FILTER_BOX_FLOATS, np.float32)
    row[0:3] = np.asarray(box.center, np.float64)
    row[3:12] = np.asarray(box.R, np.float64).T.reshape(9)
    row[12:15] = 0.5 * np.asarray(box.extent, np.float64) + float(margin)
    row[15] = 1.0
    return row


class _KeyState:
    """What ``InstanceFilter`` and ``tracking.InstanceTracker`` share: the stage events and the sorted key state (``device``, ``lib``,
    ``voxel_size``, ``keys`` and a scratch ``_keys_buf`` are the subclass's)."""

    # ---- stage timing: events on the stream, read on request ----
    def _mark(self, name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream(self.device))
        self._events.setdefault(name, []).append(ev)

    def stage_times(self) -> Dict[str, float]:
        """Milliseconds of the last ``put`` per stage, from events on the stream (waits for the device): 'kernels' (stats, decide,
        emit), 'read' (the host read of the table), 'sort_merge' (torch's unique and the segment lookup), 'search' (voxel_points
        and the box search), 'write' (the label image and the box-table rows)."""
        torch.cuda.synchronize(self.device)
        return {k: float(v[0].elapsed_time(v[1])) for k, v in self._events.items() if len(v) == 2}

    def _decode(self, keys, offsets_host):
        """(points float32 [n, 3], bounds float32 [n_seg, 6]) of sorted keys in segments."""
        n, n_seg = int(keys.numel()), len(offsets_host) - 1
        points = torch.empty(n, 3, dtype=torch.float32, device=self.device)
        bnd = torch.empty(n_seg, 6, dtype=torch.float32, device=self.device)
        off = torch.from_numpy(np.ascontiguousarray(offsets_host, np.int64)).to(self.device)
        keys = keys.contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vmapstep_voxel_points(keys.data_ptr() if n else self._keys_buf.data_ptr(), n, off.data_ptr(), n_seg,
                                                      self.voxel_size, points.data_ptr() if n else self._keys_buf.data_ptr(),
                                                      bnd.data_ptr(), _devmem.stream(self.device)), self.lib)
        return points, bnd

    def _segment(self, keys, idv):
        lo, hi = torch.searchsorted(keys, torch.tensor([idv << KEY_ID_SHIFT, (idv + 1) << KEY_ID_SHIFT], dtype=torch.int64, device=self.device)).tolist()
        return keys[lo:hi]

    def points(self, idv: int) -> torch.Tensor:
        """The cloud of one id: device float32 [n, 3], the centres of its voxels in key order."""
        seg = self._segment(self.keys, int(idv))
        return self._decode(seg, [0, int(seg.numel())])[0]


class InstanceFilter(_KeyState):
    """``InstanceFilter(width, height, intrinsics, depth_scale, max_depth, ...).put(depth, inst, sem, t_wc)``: one frame through
    ``box_filter``.  State: ``boxes`` {id: BoundingBox}, ``box_table`` (device float32 [max_ids, 16]), ``keys`` (sorted device int64)."""

    def __init__(self, width: int, height: int, intrinsics, depth_scale: float, max_depth: float,
                 background_classes=SCANNET_BACKGROUND_CLASSES, min_pixels: int = 1500, min_points: int = 10, erode_radius: int = 6,
                 voxel_size: float = 0.01, box_margin=None, id_shift: int = 1, max_ids: int = 1024, device="cuda:0"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.VmapStepError("InstanceFilter runs on the GPU (no CPU fallback): the device must be a cuda device")
        classes = [int(c) for c in background_classes]
        if len(classes) > _lib.FILTER_MAX_CLASSES:
            raise ValueError(f"at most {_lib.FILTER_MAX_CLASSES} background classes")
        if not 2 <= int(max_ids) <= _lib.FILTER_MAX_IDS:
            raise ValueError(f"max_ids must be in [2, {_lib.FILTER_MAX_IDS}]")
        if not 0 <= int(erode_radius) <= _lib.FILTER_MAX_RADIUS:
            raise ValueError(f"erode_radius must be in [0, {_lib.FILTER_MAX_RADIUS}]")
        if not float(voxel_size) > 0.0:
            raise ValueError("voxel_size must be > 0")
        self.device, self.W, self.H = dev, int(width), int(height)
        self.intrinsics = bounds._intrinsics4(intrinsics)
        self.depth_scale, self.max_depth, self.voxel_size = float(depth_scale), float(max_depth), float(voxel_size)
        self.background_classes = tuple(classes)
        self.min_pixels, self.min_points, self.erode_radius = int(min_pixels), int(min_points), int(erode_radius)
        self.box_margin = 0.875 * self.voxel_size if box_margin is None else float(box_margin)
        self.id_shift, self.max_ids = int(id_shift), int(max_ids)
        self.lib = _lib.load()
        cfg = self._cfg(False, False, np.eye(4))
        self._ws, self._ws_ptr, self._ws_bytes = _devmem.workspace(self.lib, self.lib.vmapstep_filter_workspace_bytes, dev, ctypes.byref(cfg))
        n = _lib.FILTER_HEAD_INTS + self.max_ids * _lib.FILTER_ROW_INTS
        self._rows_dev = torch.zeros(n, dtype=torch.int32, device=dev)
        self._rows_host = torch.zeros(n, dtype=torch.int32).pin_memory()
        self._status = torch.zeros(self.max_ids, dtype=torch.int32, device=dev)
        self._keys_buf = torch.zeros(self.W * self.H, dtype=torch.int64, device=dev)
        self.boxes: Dict[int, BoundingBox] = {}
        self.box_table = torch.zeros(self.max_ids, _lib.FILTER_BOX_FLOATS, dtype=torch.float32, device=dev)
        self.keys = torch.zeros(0, dtype=torch.int64, device=dev)
        self._events = {}

    def _cfg(self, depth_f32: bool, label_i32: bool, t_wc) -> _lib.FilterCfg:
        bg = (ctypes.c_int32 * 64)(*self.background_classes)
        pose = (ctypes.c_float * 16)(*np.asarray(t_wc, np.float32).reshape(16).tolist())
        fx, fy, cx, cy = self.intrinsics
        return _lib.FilterCfg(self.W, self.H, int(depth_f32), int(label_i32), self.depth_scale, self.max_depth, fx, fy, cx, cy, pose,
                              self.voxel_size, self.id_shift, self.min_pixels, self.min_points, self.erode_radius, self.max_ids,
                              len(self.background_classes), bg)

    def put(self, depth, inst, sem, t_wc) -> FilterResult:
        """One frame: depth u16 or f32 [H, W], inst and sem both u16 or both i32 [H, W], t_wc [4, 4] (camera to world).  Host tensors
        and arrays are uploaded as they are.  Raises ``ValueError`` - and leaves the state as it was - when an instance carries two
        classes or a shifted id lies outside [0, max_ids - 1]."""
        dev, H, W = self.device, self.H, self.W
        self._events = {}
        with torch.cuda.device(dev):
            depth, inst, sem = (_device_input(x, dev, n) for x, n in ((depth, "depth"), (inst, "inst"), (sem, "sem")))
            if depth is None or inst is None or sem is None:
                raise TypeError("InstanceFilter.put: depth, inst and sem are required")
            if depth.dtype not in (torch.uint16, torch.float32) or tuple(depth.shape) != (H, W):
                raise ValueError(f"depth must be uint16 or float32 [{H}, {W}], got {depth.dtype} {tuple(depth.shape)}")
            for name, t in (("inst", inst), ("sem", sem)):
                if t.dtype not in (torch.uint16, torch.int32) or tuple(t.shape) != (H, W) or t.dtype != inst.dtype:
                    raise ValueError(f"{name} must be uint16 or int32 [{H}, {W}], inst and sem of one type, got {t.dtype} {tuple(t.shape)}")
            pose = (t_wc.detach().cpu().numpy() if torch.is_tensor(t_wc) else np.asarray(t_wc)).astype(np.float32).reshape(4, 4)
            cfg = self._cfg(depth.dtype == torch.float32, inst.dtype == torch.int32, pose)
            stream = _devmem.stream(dev)
            self._mark("kernels")
            _lib.check(self.lib.vmapstep_filter_stats(ctypes.byref(cfg), depth.data_ptr(), inst.data_ptr(), sem.data_ptr(), self.box_table.data_ptr(),
                                                      self._status.data_ptr(), self._rows_dev.data_ptr(), self._ws_ptr, self._ws_bytes, stream), self.lib)
            _lib.check(self.lib.vmapstep_filter_emit(ctypes.byref(cfg), depth.data_ptr(), inst.data_ptr(), self._status.data_ptr(),
                                                     self._keys_buf.data_ptr(), self._rows_dev.data_ptr(), self._ws_ptr, self._ws_bytes, stream), self.lib)
            self._mark("kernels")
            self._mark("read")
            self._rows_host.copy_(self._rows_dev, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            self._mark("read")
            head = self._rows_host.numpy()
            n_rows, overflow, n_keys, out_of_grid = (int(x) for x in head[:_lib.FILTER_HEAD_INTS])
            if overflow:
                raise ValueError(f"{overflow} pixels carry instance ids outside [{-self.id_shift}, {self.max_ids - 1 - self.id_shift}]: "
                                 f"raise max_ids (at most {_lib.FILTER_MAX_IDS})")
            rows = head[_lib.FILTER_HEAD_INTS:_lib.FILTER_HEAD_INTS + n_rows * _lib.FILTER_ROW_INTS].reshape(n_rows, _lib.FILTER_ROW_INTS).copy()
            mixed = rows[rows[:, 1] == MIXED, 0]
            if mixed.size:
                raise ValueError(f"instance id {int(mixed[0])} carries more than one semantic class")
            touched = [int(r[0]) for r in rows if r[1] in (NEW, MERGED)]

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
                boxes = bounds.oriented_bounds(points, offsets, backend="hip", bounds=bnd, min_extent=0.0)
                found = {touched[k]: b for k, b in zip(with_keys, boxes) if b is not None}
            self._mark("search")

            res = FilterResult(torch.empty(H, W, dtype=torch.int32, device=dev), rows, out_of_grid=out_of_grid)
            no_box = []
            for r in rows:
                i, s = int(r[0]), int(r[1])
                if s == MERGED:
                    assert i in found, f"id {i}: a merged cloud contains one that had a box"
                    res.merged.append(i)
                elif s == NEW and i in found:
                    res.new.append(i)
                elif s == NEW:
                    r[1] = s = NEW_NO_BOX
                    no_box.append(i)
                res.status[i], res.classes[i], res.counts[i] = s, int(r[2]), int(r[3])
            if no_box:
                nb = torch.tensor(no_box, dtype=torch.int64, device=dev)
                self._status.index_fill_(0, nb, NEW_NO_BOX)
                keys = keys[~torch.isin(keys >> KEY_ID_SHIFT, nb)]

            # the labels against the boxes the ids had when the frame arrived; only then the new boxes
            self._mark("write")
            _lib.check(self.lib.vmapstep_filter_write(ctypes.byref(cfg), depth.data_ptr(), inst.data_ptr(), self.box_table.data_ptr(),
                                                      self._status.data_ptr(), res.labels.data_ptr(), stream), self.lib)
            if found:
                ids = sorted(found)
                table = np.stack([box_row(found[i], self.box_margin) for i in ids])
                self.box_table[torch.tensor(ids, dtype=torch.int64, device=dev)] = torch.from_numpy(table).to(dev)
            self._mark("write")
        self.keys = keys
        self.boxes.update(found)
        return res
