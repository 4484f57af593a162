"""The depth tracker on the device: the camera pose of a depth image by frame-to-model projective ICP.

Every other stage of the pipeline takes the camera-to-world pose ``t_wc`` as given.  ``track_depth`` finds it: the frame's depth image
(the SOURCE) is aligned to a depth image of the model seen from a known pose - ``raster.rasterize(mesh, pose).depth`` of the
reconstruction, ``render_view(...).depth`` of the fields, or simply the previous frame - by point-to-plane ICP with projective
association, coarse to fine over a depth pyramid.  ``DepthTracker`` keeps the model and the last pose from frame to frame.

The rules are csrc/icp_rules.h's, the kernels csrc/icp_kernels.h's (unit k_icp.hip), the contract the icp section of
include/vmapstep.h; it is this project's own.  Images are ``[W, H]`` float32, width-major, as ``FrameStore`` holds them.  The state
of the iteration is T, the source-camera -> model-camera matrix in float64; all sums are integer (each addend quantised to 2^-30),
so a call's result is a function of its input alone, bit for bit, whatever the schedule.  GPU only; there is no CPU fallback.

No colour term, no loop closure, no keyframe policy, no motion model: the caller decides what the model is and when to replace it."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _devmem, _lib
from .bounds import _intrinsics4

__all__ = ["DepthMaps", "TrackedPose", "DepthTracker", "depth_maps", "icp_sums", "track_depth", "level_sizes"]

OK, DEGENERATE, SKIPPED = _lib.ICP_OK, _lib.ICP_DEGENERATE, _lib.ICP_SKIPPED
DEFAULTS = dict(dist_thresh=0.15, cos_thresh=0.8, band=0.25, min_depth=0.1, max_depth=10.0, damping=0.0, pivot_rel=1e-3, eps=1e-6, min_inliers=12)


def level_sizes(width, height, levels):
    """[(W_l, H_l)] of a pyramid: W_l+1 = ceil(W_l / 2)."""
    out = []
    for _ in range(int(levels)):
        out.append((int(width), int(height)))
        width, height = (int(width) + 1) // 2, (int(height) + 1) // 2
    return out


@dataclass
class DepthMaps:
    """The pyramid of one depth image.  ``entries[l]`` is float32 ``[W_l, H_l, 4]`` = (n0, n1, n2, d) per pixel, views of ONE device
    buffer (``buffer``); ``depth[l]`` / ``normals[l]`` / ``valid[l]`` / ``has_normal[l]`` are read from it."""
    buffer: torch.Tensor
    entries: List[torch.Tensor]
    cfg: dict

    @property
    def depth(self):
        return [e[..., 3] for e in self.entries]

    @property
    def normals(self):
        return [e[..., :3] for e in self.entries]

    @property
    def valid(self):
        return [e[..., 3] > 0 for e in self.entries]

    @property
    def has_normal(self):
        return [(e[..., :3] != 0).any(-1) for e in self.entries]


@dataclass
class TrackedPose:
    t_wc: torch.Tensor                         # float32 [4, 4] on the device: t_wc64 rounded
    t_wc64: np.ndarray                         # float64 [4, 4] = t_wc_model @ T
    t_sm64: np.ndarray                         # float64 [4, 4]: T, source camera -> model camera, as the device left it
    log: np.ndarray                            # float64 [n_iter, 4]: inlier count, sum of r^2, status, |x|^2; coarse level first
    sums: np.ndarray                           # int64 [n_iter, 29]
    poses: np.ndarray                          # float64 [n_iter, 12]: T after every iteration
    ok: bool                                   # the last iteration of level 0 that ran was not DEGENERATE
    inlier_fraction: float                     # its inlier count / (W * H)


def _device():
    if not torch.cuda.is_available():
        raise _lib.VmapStepError("the depth tracker runs on the GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _cfg(intrinsics, width, height, levels, iterations=None, grid_cap=0, **kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown arguments {sorted(unknown)}")
    missing = [k for k in DEFAULTS if kw.get(k) is None]
    if missing:
        raise TypeError(f"missing arguments {missing}")
    levels = int(levels)
    if not 1 <= levels <= _lib.ICP_MAX_LEVELS:
        raise _lib.VmapStepError(f"icp: levels must be in 1 .. {_lib.ICP_MAX_LEVELS}")
    its = [0] * _lib.ICP_MAX_LEVELS
    if iterations is not None:
        if len(iterations) != levels:
            raise _lib.VmapStepError("icp: one iteration count per level, coarse first")
        for level, n in enumerate(reversed(list(iterations))):          # coarse first -> index 0 = the finest
            its[level] = int(n)
    fx, fy, cx, cy = _intrinsics4(intrinsics)
    return _lib.IcpCfg(int(width), int(height), levels, int(kw["min_inliers"]), (ctypes.c_int32 * 4)(*its), int(grid_cap), 0, fx, fy, cx, cy,
                       float(kw["min_depth"]), float(kw["max_depth"]), float(kw["band"]), float(kw["dist_thresh"]), float(kw["cos_thresh"]), 0.0,
                       float(kw["damping"]), float(kw["pivot_rel"]), float(kw["eps"]))


def _image(depth, dev):
    d = torch.as_tensor(depth).to(device=dev, dtype=torch.float32).contiguous()
    if d.dim() != 2 or d.numel() == 0:
        raise _lib.VmapStepError("icp: a depth image is [W, H]")
    return d


def _build_maps(lib, cfg, depth, dev):
    nb = ctypes.c_size_t()
    _lib.check(lib.vmapstep_icp_maps_bytes(ctypes.byref(cfg), ctypes.byref(nb)), lib)
    buf = torch.empty(nb.value // 4, dtype=torch.float32, device=dev)
    _lib.check(lib.vmapstep_icp_pyramid(ctypes.byref(cfg), depth.data_ptr(), buf.data_ptr(), _devmem.stream(dev)), lib)
    entries, at = [], 0
    for w, h in level_sizes(cfg.width, cfg.height, cfg.levels):
        entries.append(buf[at:at + w * h * 4].view(w, h, 4))
        at += w * h * 4
    return buf, entries


def depth_maps(depth, intrinsics, levels=3, *, min_depth, max_depth, band):
    """The pyramid of ``depth`` ([W, H] float32, host or device) as ``DepthMaps``: per level the depth (0 = invalid: not finite, not in
    ``(min_depth, max_depth]``, or a 2 x 2 block whose valid depths span more than ``band``), the camera-frame normals towards the
    camera ((0, 0, 0) = none: a border pixel, an invalid neighbour, or a central difference in depth above ``2 * band``) and the two
    validity masks.  Level l + 1 is ``ceil(W_l / 2) x ceil(H_l / 2)`` with the camera ``fx / 2^l``, ``(cx - (2^l - 1) / 2) / 2^l``."""
    dev = _device()
    lib = _lib.load()
    d = _image(depth, dev)
    kw = dict(DEFAULTS, min_depth=min_depth, max_depth=max_depth, band=band)
    cfg = _cfg(intrinsics, d.shape[0], d.shape[1], levels, **kw)
    buf, entries = _build_maps(lib, cfg, d, dev)
    return DepthMaps(buf, entries, dict(intrinsics=_intrinsics4(intrinsics), levels=int(levels), min_depth=min_depth, max_depth=max_depth, band=band))


def _rows12(t):
    t = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64)
    if t.size == 16:
        t = t.reshape(4, 4)[:3]
    if t.size != 12 or not np.isfinite(t).all():
        raise _lib.VmapStepError("icp: a pose is a finite [4, 4] or [3, 4] matrix")
    return np.ascontiguousarray(t.reshape(12))


def icp_sums(src_maps, model_maps, level, t_sm, *, dist_thresh=DEFAULTS["dist_thresh"], cos_thresh=DEFAULTS["cos_thresh"], grid_cap=0):
    """One iteration's reduction at ``level`` under the pose ``t_sm`` (source camera -> model camera): int64 [29] on the device - the
    inlier count, the 21 upper entries of J J^T, the 6 of J r, and r^2, each addend rint(x * 2^30).  ``src_maps`` / ``model_maps``:
    two ``depth_maps`` results of one size and one configuration.  For tests; ``track_depth`` runs the whole chain."""
    dev = _device()
    lib = _lib.load()
    if src_maps.cfg != model_maps.cfg or src_maps.buffer.shape != model_maps.buffer.shape:
        raise _lib.VmapStepError("icp_sums: the two pyramids must share one size and one configuration")
    c = src_maps.cfg
    w, h = src_maps.entries[0].shape[:2]
    cfg = _cfg(c["intrinsics"], w, h, c["levels"], grid_cap=grid_cap,
               **dict(DEFAULTS, min_depth=c["min_depth"], max_depth=c["max_depth"], band=c["band"], dist_thresh=dist_thresh, cos_thresh=cos_thresh))
    pose = torch.from_numpy(_rows12(t_sm)).to(dev)
    out = torch.empty(_lib.ICP_SUMS, dtype=torch.int64, device=dev)
    _lib.check(lib.vmapstep_icp_sums(ctypes.byref(cfg), src_maps.buffer.data_ptr(), model_maps.buffer.data_ptr(), int(level), pose.data_ptr(),
                                     out.data_ptr(), _devmem.stream(dev)), lib)
    return out


def _rigid_inverse(t):
    out = np.eye(4)
    out[:3, :3] = t[:3, :3].T
    out[:3, 3] = -t[:3, :3].T @ t[:3, 3]
    return out


def _pose44(t):
    out = np.eye(4)
    out[:3] = _rows12(t).reshape(3, 4)
    return out


def _track(lib, cfg, dev, src_buf, model_buf, t_wc_model, t_wc_init):
    t_model, t_init = _pose44(t_wc_model), _pose44(t_wc_init)
    n = sum(cfg.iterations[level] for level in range(cfg.levels))
    pose = torch.from_numpy(np.ascontiguousarray((_rigid_inverse(t_model) @ t_init)[:3].reshape(12))).to(dev)
    # one buffer for everything the host reads back: the pose [12], the log [n, 4], the pose log [n, 12] (float64), the sums log [n, 29]
    out = torch.zeros(12 + n * (4 + 12 + 29), dtype=torch.float64, device=dev)
    out[:12] = pose
    state, state_ptr = _devmem.aligned(_lib.ICP_STATE_BYTES, dev)
    base = out.data_ptr()
    _lib.check(lib.vmapstep_icp_track(ctypes.byref(cfg), src_buf.data_ptr(), model_buf.data_ptr(), base, base + 8 * 12, base + 8 * (12 + 16 * n),
                                      base + 8 * (12 + 4 * n), state_ptr, _devmem.stream(dev)), lib)
    host = out.cpu().numpy()                                           # the one host synchronisation of the call
    del state
    T = np.eye(4)
    T[:3] = host[:12].reshape(3, 4)
    log = host[12:12 + 4 * n].reshape(n, 4).copy()
    poses = host[12 + 4 * n:12 + 16 * n].reshape(n, 12).copy()
    sums = host[12 + 16 * n:].view(np.int64).reshape(n, 29).copy()
    level0 = log[n - cfg.iterations[0]:]
    live = level0[level0[:, 2] != SKIPPED]
    last = live[-1]
    t_wc64 = t_model @ T
    return TrackedPose(torch.from_numpy(t_wc64.astype(np.float32)).to(dev), t_wc64, T, log, sums, poses, bool(int(last[2]) == OK),
                       float(last[0]) / (cfg.width * cfg.height))


def track_depth(depth, model_depth, t_wc_model, t_wc_init, intrinsics, *, iterations=(10, 5, 4), dist_thresh, cos_thresh, band, min_depth,
                max_depth, damping=0.0, pivot_rel, eps, min_inliers, grid_cap=0):
    """The camera-to-world pose of ``depth`` from its alignment to ``model_depth``, a depth image of the same size and camera seen from
    ``t_wc_model``; ``t_wc_init`` is the first guess.  -> ``TrackedPose``.

    Both images are brought to the model camera: the state is T, the matrix that takes a point of the source camera's frame to the
    model camera's frame, float64, starting at ``inverse(t_wc_model) @ t_wc_init``.  An iteration transforms every source point with
    a normal by T, projects it into the model image (nearest pixel), keeps the pair if the model pixel has a normal, the depths differ
    by at most ``dist_thresh`` and the normals' cosine is at least ``cos_thresh``, solves the point-to-plane normal equations (LDL^T,
    ``damping`` added to the diagonal) for x = (v, omega) and sets T <- dT @ T with the Cayley rotation of omega / 2 and the
    translation v.  ``iterations``: per level, COARSE FIRST (its length is the number of levels).  A level ends early once
    |x|^2 < ``eps``^2 (its remaining rows are SKIPPED); an iteration is DEGENERATE, and leaves T alone, with fewer than
    ``min_inliers`` pairs or a pivot <= ``pivot_rel`` * the largest diagonal entry.

    The returned pose is exactly ``t_wc64 = t_wc_model @ T`` in float64 on the host (a source point p is at T p in the model camera
    and so at t_wc_model T p in the world), ``t_wc`` its float32 rounding on the device.  ``ok`` is false if the last iteration of
    level 0 that ran was DEGENERATE.  One host synchronisation, at the end.  ``grid_cap`` is for tests (a small reduction grid)."""
    dev = _device()
    lib = _lib.load()
    d, m = _image(depth, dev), _image(model_depth, dev)
    if d.shape != m.shape:
        raise _lib.VmapStepError("track_depth: depth and model_depth must have one shape")
    cfg = _cfg(intrinsics, d.shape[0], d.shape[1], len(iterations), iterations, grid_cap, dist_thresh=dist_thresh, cos_thresh=cos_thresh, band=band,
               min_depth=min_depth, max_depth=max_depth, damping=damping, pivot_rel=pivot_rel, eps=eps, min_inliers=min_inliers)
    _rows12(t_wc_model), _rows12(t_wc_init)                            # refused before anything is enqueued
    src, _ = _build_maps(lib, cfg, d, dev)
    mod, _ = _build_maps(lib, cfg, m, dev)
    return _track(lib, cfg, dev, src, mod, t_wc_model, t_wc_init)


class DepthTracker:
    """Frame-to-model tracking with a kept model and a kept pose.

    ``DepthTracker(intrinsics, width, height, iterations=(10, 5, 4), **cfg)`` (``cfg``: ``track_depth``'s keyword arguments; unset
    ones take ``odometry.DEFAULTS``); ``set_model(depth, t_wc)`` builds the model's pyramid once; ``track(depth, t_wc_init=None)``
    aligns a frame to it (the default first guess is the last pose) and, on ``ok``, advances the last pose.  A refused call leaves
    the model and the last pose as they were."""

    def __init__(self, intrinsics, width, height, iterations=(10, 5, 4), grid_cap=0, **cfg):
        self.intrinsics = _intrinsics4(intrinsics)
        self.width, self.height = int(width), int(height)
        self.iterations = tuple(int(n) for n in iterations)
        self.params = dict(DEFAULTS, **cfg)
        self._cfg = _cfg(self.intrinsics, self.width, self.height, len(self.iterations), self.iterations, grid_cap, **self.params)
        nb = ctypes.c_size_t()
        _lib.check(_lib.load().vmapstep_icp_maps_bytes(ctypes.byref(self._cfg), ctypes.byref(nb)), _lib.load())
        self._model = None
        self.t_wc_model: Optional[np.ndarray] = None
        self.t_wc: Optional[np.ndarray] = None                         # the last pose, float64 [4, 4]

    def _check(self, depth, dev):
        d = _image(depth, dev)
        if tuple(d.shape) != (self.width, self.height):
            raise _lib.VmapStepError(f"DepthTracker: a depth image is [{self.width}, {self.height}]")
        return d

    def set_model(self, depth, t_wc):
        dev = _device()
        d = self._check(depth, dev)
        t = _pose44(t_wc)
        model, _ = _build_maps(_lib.load(), self._cfg, d, dev)
        self._model, self.t_wc_model = model, t
        if self.t_wc is None:
            self.t_wc = t.copy()

    def track(self, depth, t_wc_init=None):
        dev = _device()
        if self._model is None:
            raise _lib.VmapStepError("DepthTracker.track: set_model first")
        d = self._check(depth, dev)
        init = self.t_wc if t_wc_init is None else _pose44(t_wc_init)
        lib = _lib.load()
        src, _ = _build_maps(lib, self._cfg, d, dev)
        res = _track(lib, self._cfg, dev, src, self._model, self.t_wc_model, init)
        if res.ok:
            self.t_wc = res.t_wc64.copy()
        return res

    def track_to_mesh(self, mesh, depth, *, min_raster_depth=None):
        """Rasterises ``mesh`` at the last pose (``raster.rasterize``), makes that the model, then tracks ``depth`` against it."""
        from . import raster
        if self.t_wc is None:
            raise _lib.VmapStepError("DepthTracker.track_to_mesh: no pose yet (set_model, or set t_wc)")
        dev = _device()
        self._check(depth, dev)
        near = float(self.params["min_depth"]) if min_raster_depth is None else float(min_raster_depth)
        r = raster.rasterize(mesh, self.t_wc.astype(np.float32)[None], self.intrinsics, self.width, self.height, min_depth=near)
        # the raster drew from the float32 rounding of the pose: that rounding is the model's pose
        self.set_model(r.depth[0], self.t_wc.astype(np.float32).astype(np.float64))
        return self.track(depth)

    def track_to_volume(self, volume, depth, **raycast_kw):
        """Ray-casts a ``tsdf.TSDFVolume`` at the last pose (``TSDFVolume.raycast``; ``raycast_kw`` goes to it, ``min_depth`` and
        ``max_depth`` default to the tracker's own), makes that the model, then tracks ``depth`` against it."""
        if self.t_wc is None:
            raise _lib.VmapStepError("DepthTracker.track_to_volume: no pose yet (set_model, or set t_wc)")
        dev = _device()
        self._check(depth, dev)
        raycast_kw.setdefault("min_depth", float(self.params["min_depth"]))
        raycast_kw.setdefault("max_depth", float(self.params["max_depth"]))
        raycast_kw.setdefault("normals", False)
        view = volume.raycast(self.t_wc, self.intrinsics, self.width, self.height, **raycast_kw)
        # the volume was cast from the float32 rounding of the pose: that rounding is the model's pose
        self.set_model(view.depth[0], view.t_wc[0].astype(np.float64))
        return self.track(depth)

    def track_to_view(self, view, depth, min_opacity, t_wc=None):
        """Tracks ``depth`` against a ``render.View``'s depth image, zeroed where its opacity is below ``min_opacity``; ``t_wc``: the
        pose the view was rendered from (default: the last pose)."""
        dev = _device()
        self._check(depth, dev)
        pose = self.t_wc if t_wc is None else _pose44(t_wc)
        if pose is None:
            raise _lib.VmapStepError("DepthTracker.track_to_view: no pose")
        model = torch.where(view.opacity >= float(min_opacity), view.depth, torch.zeros_like(view.depth))
        self.set_model(model, pose)
        return self.track(depth)
