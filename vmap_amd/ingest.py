"""Frame ingest on the device: a decoded frame into a ``FrameStore`` slot, with the objects in it and their 2-D boxes
(csrc/ingest_kernels.h, csrc/ingest_rules.h; the contract is the ingest section of include/vmapstep.h).

The reference does this on the host once per frame: the labelling part of ``Replica.__getitem__`` (dataset.py:93-133: one full-frame
mask per instance, the class filter, ``get_bbox2d_batch`` + ``enlarge_bbox``, the relabel), the depth transform
(image_transforms.py:13-33) and the transposes to [W, H] (dataset.py:87-91) - and the caller then hands the result to its keyframe
buffers.  ``FrameIngest.put`` takes the frame as the image files hold it (row-major [H, W]) and does all of it in four launches on
the current stream; the read of the small object table is its only synchronisation.  GPU only: there is no eager path.

With ``background_classes=()``, ``min_box=-1`` and ``sem=None`` the same call does the second half of ``ScanNet.__getitem__``
(dataset.py:266-274) on a label image that ``box_filter`` has already merged - on the assumption that ``cv2.boundingRect`` over all
external contours is the mask's min / max extent plus one, which could not be checked against OpenCV where this was written.
``box_filter`` itself is ``vmap_amd.instances.InstanceFilter.put``, whose ``labels`` go straight into this call.  Reading and decoding
the image files and the keyframe policy stay with the caller; ``track_instance`` is ``vmap_amd.tracking.InstanceTracker.put``.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List

import numpy as np
import torch

from . import _devmem, _lib
from .keyframes import FrameStore

__all__ = ["FrameIngest", "IngestResult", "REPLICA_BACKGROUND_CLASSES", "SCANNET_BACKGROUND_CLASSES", "STATUS_NAMES"]

# the two lists of the reference's loaders (dataset.py:74, 187): settings
REPLICA_BACKGROUND_CLASSES = (5, 12, 30, 31, 40, 60, 92, 93, 95, 97, 98, 79)
SCANNET_BACKGROUND_CLASSES = (-1, 0, 1, 3, 16, 41, 232, 21, 161, 128, 21)

ABSENT, KEPT, BACKGROUND, SMALL, ZERO_MARGIN, MIXED = range(6)
STATUS_NAMES = ("ABSENT", "KEPT", "BACKGROUND", "SMALL", "ZERO_MARGIN", "MIXED")
MAX_IDS_LIMIT = 65537


@dataclass
class IngestResult:
    slot: int                              # the FrameStore slot (reference count 0, as FrameStore.put returns it)
    ids: List[int]                         # ascending: 0 and every KEPT id - the keys of the reference's bbox_dict
    bbox: Dict[int, torch.Tensor]          # id -> float32 [4] (u low, u high, v low, v high), for ObjectKeyframes / ok.write
    counts: Dict[int, int]                 # every id present in the frame (and 0) -> its pixels
    status: Dict[int, int]                 # every id present in the frame (and 0) -> KEPT, BACKGROUND, SMALL, ZERO_MARGIN (ABSENT: id 0 only)
    classes: Dict[int, int]                # every id present -> its class
    rows: np.ndarray                       # int32 [n, 8]: id, status, count, box[4], class in ascending id


def _device_input(x, device, what):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not torch.is_tensor(t):
        raise TypeError(f"FrameIngest.put: {what} must be a tensor or an array")
    return t.to(device, non_blocking=True).contiguous()       # uploaded as it is: 16-bit stays 16-bit


class FrameIngest:
    """``FrameIngest(store, depth_scale, max_depth, ...).put(rgb, depth, inst, sem, t_wc, frame_id)``: one frame into ``store``."""

    def __init__(self, store: FrameStore, depth_scale: float, max_depth: float, background_classes=(), bbox_scale: float = 0.2,
                 min_box: int = 10, max_ids: int = 1024):
        if store.device.type != "cuda":
            raise _lib.VmapStepError("FrameIngest runs on the GPU (no CPU fallback): the store must live on a cuda device")
        classes = [int(c) for c in background_classes]
        if len(classes) > _lib.INGEST_MAX_CLASSES:
            raise ValueError(f"at most {_lib.INGEST_MAX_CLASSES} background classes")
        if not 2 <= int(max_ids) <= MAX_IDS_LIMIT:
            raise ValueError(f"max_ids must be in [2, {MAX_IDS_LIMIT}]")
        if not float(bbox_scale) >= 0.0:
            raise ValueError("bbox_scale must be >= 0")
        self.store = store
        self.depth_scale, self.max_depth, self.bbox_scale = float(depth_scale), float(max_depth), float(bbox_scale)
        self.min_box, self.max_ids, self.background_classes = int(min_box), int(max_ids), tuple(classes)
        self.lib = _lib.load()
        dev = store.device
        self._ws, self._ws_ptr, self._ws_bytes = _devmem.workspace(self.lib, self.lib.vmapstep_ingest_workspace_bytes, dev, self.max_ids)
        n = 2 + self.max_ids * _lib.INGEST_ROW_INTS
        self._rows_dev = torch.zeros(n, dtype=torch.int32, device=dev)
        self._rows_host = torch.zeros(n, dtype=torch.int32).pin_memory()

    def _cfg(self, depth_f32: bool, label_i32: bool) -> _lib.IngestCfg:
        bg = (ctypes.c_int32 * 64)(*self.background_classes)
        return _lib.IngestCfg(self.store.W, self.store.H, int(depth_f32), int(label_i32), self.depth_scale, self.max_depth, self.bbox_scale,
                              self.min_box, self.max_ids, len(self.background_classes), bg)

    def enqueue(self, slot: int, rgb, depth, inst, sem):
        """The four launches for device tensors, into ``slot``; nothing waits.  The table lands in ``self._rows_dev``."""
        st = self.store
        H, W = st.H, st.W
        if rgb.dtype != torch.uint8 or tuple(rgb.shape) != (H, W, 3):
            raise ValueError(f"rgb must be uint8 [{H}, {W}, 3], got {rgb.dtype} {tuple(rgb.shape)}")
        if depth.dtype not in (torch.uint16, torch.float32) or tuple(depth.shape) != (H, W):
            raise ValueError(f"depth must be uint16 or float32 [{H}, {W}], got {depth.dtype} {tuple(depth.shape)}")
        label_i32 = False
        if inst is None:
            if sem is not None:
                raise ValueError("sem without inst")
        else:
            for name, t in (("inst", inst), ("sem", sem)):
                if t is not None and (t.dtype not in (torch.uint16, torch.int32) or tuple(t.shape) != (H, W) or t.dtype != inst.dtype):
                    raise ValueError(f"{name} must be uint16 or int32 [{H}, {W}], inst and sem of one type, got {t.dtype} {tuple(t.shape)}")
            label_i32 = inst.dtype == torch.int32
        cfg = self._cfg(depth.dtype == torch.float32, label_i32)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self.lib.vmapstep_ingest_frame(ctypes.byref(cfg), rgb.data_ptr(), depth.data_ptr(), ptr(inst), ptr(sem),
                                                  st.rgbx[slot].data_ptr(), st.depth[slot].data_ptr(), st.inst[slot].data_ptr(),
                                                  self._rows_dev.data_ptr(), self._ws_ptr, self._ws_bytes, _devmem.stream(st.device)), self.lib)

    def put(self, rgb, depth, inst, sem, t_wc, frame_id: int) -> IngestResult:
        """Store one frame: rgb u8 [H, W, 3], depth u16 or f32 [H, W], inst and sem u16 or i32 [H, W] (``inst=None``: no labels, the
        reference's imap_mode; ``sem=None``: no class filter), t_wc [4, 4].  Host tensors and arrays are uploaded as they are.  The slot
        is chosen as ``FrameStore.put`` chooses it and comes back with a reference count of 0.  Raises ``ValueError`` - and leaves the
        slot free - when an instance carries two classes (as the reference does) or an id lies outside [-1, max_ids - 2]."""
        st = self.store
        dev = st.device
        slot = st.free_slot()
        with torch.cuda.device(dev):
            rgb, depth, inst, sem = (_device_input(x, dev, n) for x, n in ((rgb, "rgb"), (depth, "depth"), (inst, "inst"), (sem, "sem")))
            self.enqueue(slot, rgb, depth, inst, sem)
            st.t_wc[slot].copy_(torch.as_tensor(np.asarray(t_wc) if not torch.is_tensor(t_wc) else t_wc).to(dev, torch.float32, non_blocking=True))
            self._rows_host.copy_(self._rows_dev, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()          # the call's only synchronisation
        head = self._rows_host.numpy()
        n_rows, overflow = int(head[0]), int(head[1])
        if overflow:
            raise ValueError(f"{overflow} pixels carry instance ids outside [-1, {self.max_ids - 2}]: raise max_ids (at most {MAX_IDS_LIMIT})")
        rows = head[2:2 + n_rows * _lib.INGEST_ROW_INTS].reshape(n_rows, _lib.INGEST_ROW_INTS).copy()
        mixed = rows[rows[:, 1] == MIXED, 0]
        if mixed.size:
            raise ValueError(f"instance id {int(mixed[0])} carries more than one semantic class")
        res = IngestResult(slot, [], {}, {}, {}, {}, rows)
        for i, s, c, b0, b1, b2, b3, k in rows.tolist():
            res.counts[i], res.status[i], res.classes[i] = c, s, k
            if s == KEPT or i == 0:
                res.ids.append(i)
                res.bbox[i] = torch.tensor([b0, b1, b2, b3], dtype=torch.float32)
        st.frame_of_slot[slot] = int(frame_id)
        return res
