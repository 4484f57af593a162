"""The mesh rasteriser on the device: what a camera at each of a set of poses sees of a triangle mesh.

``rasterize`` gives, per view and pixel, the depth along the optical axis and the face that is nearest there - a depth stack in the
layout ``visibility.mark_visible`` and ``FrameStore`` use, and, with per-face labels, an instance image ``FrameIngest.put`` accepts.
``visible_faces`` / ``cull_to_raster`` keep the faces that won a pixel in some view: the exact form of visibility culling, which
``visibility.cull_to_views`` approximates by a face's corners.  ``compare_depth`` / ``depth_l1`` give Depth L1, the 2-D metric of
iMAP and NICE-SLAM: the mean absolute difference between depth images of the reconstruction and of the ground truth from the same
poses.  The rule is csrc/raster_rules.h's, the kernels csrc/raster_kernels.h's, the contract the raster section of include/vmapstep.h;
it is this project's own.

The known limit: there is no near-plane clipping.  A face with a corner at or behind ``min_depth`` (or outside a guard band of
16384 pixels) is dropped from that view whole and counted in ``Raster.dropped`` - harmless for meshes whose triangles are small
against their distance (marching-cubes output, scanned ground truth), wrong for a room made of twelve triangles seen from inside."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _devmem, _lib
from .bounds import _intrinsics4
from .meshing import Mesh
from .visibility import _slots

__all__ = ["Raster", "rasterize", "visible_faces", "cull_mesh_faces", "cull_to_raster", "compare_depth", "depth_l1"]

DEFAULT_BUDGET = 256 << 20                     # bytes of key images per chunk of views: 39 views of 1200 x 680


@dataclass
class Raster:
    depth: torch.Tensor                        # float32 [K, W, H]; 0 where nothing was drawn
    face: torch.Tensor                         # int32 [K, W, H]; -1 where nothing was drawn
    label: Optional[torch.Tensor]              # int32 [K, W, H] = face_labels[face], -1 where nothing was drawn; None without face_labels
    dropped: torch.Tensor                      # int32 [K]: faces that took no part in the view (see the module's docstring)


def _device():
    if not torch.cuda.is_available():
        raise _lib.VmapStepError("the mesh rasteriser runs on the GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _mesh_arrays(mesh, dev):
    v, f = (mesh.vertices, mesh.faces) if hasattr(mesh, "vertices") else mesh
    v = torch.as_tensor(v).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    f = torch.as_tensor(f).to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    return v, f


def _draw(mesh, t_wc, intrinsics, width, height, min_depth, max_depth, slots, budget_bytes, resolve):
    """Draws the views in chunks whose key images fit ``budget_bytes`` and hands every chunk to ``resolve(keys, k0, k1)``.  A view's
    key image depends on that view alone, so the chunking cannot show in the result.  -> dropped int32 [K]"""
    lib = _lib.load()
    dev = _device()
    v, f = _mesh_arrays(mesh, dev)
    poses = torch.as_tensor(t_wc).to(device=dev, dtype=torch.float32).reshape(-1, 4, 4).contiguous()
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise _lib.VmapStepError("rasterize: width and height must be positive")
    if min_depth is None or not float(min_depth) > 0:
        raise _lib.VmapStepError("rasterize: min_depth must be > 0")
    sl, K = _slots(slots, int(poses.shape[0]), dev)
    if sl is None:
        sl = torch.arange(K, dtype=torch.int32, device=dev)
    fx, fy, cx, cy = _intrinsics4(intrinsics)
    cfg = _lib.RasterCfg(fx, fy, cx, cy, float(min_depth), float(max_depth) if max_depth else 0.0, width, height)
    dropped = torch.zeros(K, dtype=torch.int32, device=dev)
    per = max(1, min(int(budget_bytes) // (width * height * 8), 65535))
    stream = _devmem.stream(dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    for k0 in range(0, K, per):
        k1 = min(K, k0 + per)
        n = k1 - k0
        keys = torch.empty((n, width, height), dtype=torch.int64, device=dev)
        nws, nlarge = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.vmapstep_raster_workspace_bytes(len(f), n, 0, ctypes.byref(nws), ctypes.byref(nlarge)), lib)
        ws, ws_ptr = _devmem.aligned(nws.value, dev)
        mesh_views = (ctypes.byref(cfg), v.data_ptr(), len(v), f.data_ptr(), len(f), poses.data_ptr(), sl[k0:k1].data_ptr(), n, keys.data_ptr())
        _lib.check(lib.vmapstep_raster_count(*mesh_views, dropped[k0:k1].data_ptr(), counts.data_ptr(), ws_ptr, nws.value, stream), lib)
        n_large, n_pairs = (int(x) for x in counts.cpu())          # the one host synchronisation of the chunk
        if n_large > 0:
            _lib.check(lib.vmapstep_raster_workspace_bytes(len(f), n, n_large, ctypes.byref(nws), ctypes.byref(nlarge)), lib)
            large, large_ptr = _devmem.aligned(nlarge.value, dev)
            _lib.check(lib.vmapstep_raster_draw(*mesh_views, n_large, n_pairs, large_ptr, n_large, nlarge.value, ws_ptr, nws.value, stream), lib)
            del large
        resolve(lib, keys, k0, k1, len(f), stream)
        del ws, keys
    return dropped


def rasterize(mesh, t_wc, intrinsics, width, height, *, min_depth, max_depth=None, face_labels=None, slots=None,
              budget_bytes=DEFAULT_BUDGET):
    """Depth and face images of ``mesh`` (a ``meshing.Mesh`` or a ``(vertices, faces)`` pair) from the poses ``t_wc`` [K, 4, 4]
    (camera to world, rotations assumed orthonormal), as a ``Raster`` of [K, W, H] device tensors, width-major.

    ``intrinsics``: (fx, fy, cx, cy), a 3 x 3 matrix or an object with those attributes; pixel (w, h) has its centre at u = w, v = h.
    ``min_depth`` (> 0, required): a face takes part in a view only if every corner lies farther than that along the optical axis -
    there is no near-plane clipping; ``Raster.dropped`` counts the faces a view lost.  ``max_depth``: pixels farther than that stay
    empty.  ``face_labels`` (int [F]): also return ``label = face_labels[face]``.  ``slots``: the views to draw, as indices into
    ``t_wc`` (default: all, in order).  Views are drawn in chunks whose z-buffers (8 bytes per pixel) fit ``budget_bytes``; the result
    is bit-identical whatever the chunking, and from run to run.  One host synchronisation per chunk."""
    dev = _device()
    K = len(slots) if slots is not None else int(torch.as_tensor(t_wc).reshape(-1, 4, 4).shape[0])
    depth = torch.zeros((K, int(width), int(height)), dtype=torch.float32, device=dev)
    face = torch.full((K, int(width), int(height)), -1, dtype=torch.int32, device=dev)
    labels = label = None
    if face_labels is not None:
        labels = torch.as_tensor(face_labels).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        n_faces = len(mesh.faces if hasattr(mesh, "faces") else mesh[1])
        if labels.numel() != n_faces:
            raise _lib.VmapStepError("rasterize: one label per face")
        label = torch.full_like(face, -1)

    def resolve(lib, keys, k0, k1, n_faces, stream):
        _lib.check(lib.vmapstep_raster_resolve(keys.data_ptr(), keys.numel(), depth[k0:k1].data_ptr(), face[k0:k1].data_ptr(),
                                               None if labels is None else labels.data_ptr(), n_faces,
                                               None if label is None else label[k0:k1].data_ptr(), None, stream), lib)

    dropped = _draw(mesh, t_wc, intrinsics, width, height, min_depth, max_depth, slots, budget_bytes, resolve)
    return Raster(depth, face, label, dropped)


def visible_faces(mesh, t_wc, intrinsics, width, height, *, min_depth, max_depth=None, slots=None, seen=None, budget_bytes=DEFAULT_BUDGET):
    """uint8 device tensor [F]: 1 for every face that won at least one pixel in some view (``rasterize``'s arguments).  ``seen``: a
    mask from an earlier call to add to - the call only ever turns a 0 into a 1, so views may be marked in several calls."""
    dev = _device()
    n_faces = len(mesh.faces if hasattr(mesh, "faces") else mesh[1])
    if seen is None:
        seen = torch.zeros(n_faces, dtype=torch.uint8, device=dev)
    elif not (isinstance(seen, torch.Tensor) and seen.dtype == torch.uint8 and seen.device == dev and seen.is_contiguous() and seen.numel() == n_faces):
        raise _lib.VmapStepError("visible_faces: seen must be a contiguous uint8 tensor [F] on the device")

    def resolve(lib, keys, k0, k1, n_faces, stream):
        scratch_d = torch.empty(keys.shape, dtype=torch.float32, device=dev)
        scratch_f = torch.empty(keys.shape, dtype=torch.int32, device=dev)
        _lib.check(lib.vmapstep_raster_resolve(keys.data_ptr(), keys.numel(), scratch_d.data_ptr(), scratch_f.data_ptr(), None, n_faces, None,
                                               seen.data_ptr() if n_faces else None, stream), lib)

    _draw(mesh, t_wc, intrinsics, width, height, min_depth, max_depth, slots, budget_bytes, resolve)
    return seen


def cull_mesh_faces(mesh, face_mask):
    """The faces of ``mesh`` the mask keeps (non-zero = keep, one entry per face) and the vertices they reference, as a ``Mesh``, or
    ``None`` when no face is left.  ``visibility.cull_mesh``'s order contract: faces keep their order, vertices their ascending
    order, normals and colours travel with their vertices.  Torch indexing: this is not a hot path."""
    dev = _device()
    v, f = _mesh_arrays(mesh, dev)
    keep = torch.as_tensor(face_mask).to(dev).reshape(-1) != 0
    if keep.numel() != len(f):
        raise _lib.VmapStepError("cull_mesh_faces: one mask entry per face")
    keep &= ((f >= 0) & (f < len(v))).all(1)               # a face with an index out of range is never drawn, and never kept
    kf = f[keep].long()
    if len(kf) == 0:
        return None
    used = torch.zeros(len(v), dtype=torch.bool, device=dev)
    used[kf.reshape(-1)] = True
    idx = torch.nonzero(used).reshape(-1)                  # ascending
    new = torch.full((len(v),), -1, dtype=torch.int32, device=dev)
    new[idx] = torch.arange(len(idx), dtype=torch.int32, device=dev)
    gather = lambda t: None if t is None else torch.as_tensor(t).to(dev)[idx]
    return Mesh(v[idx], new[kf], gather(getattr(mesh, "vertex_normals", None)), gather(getattr(mesh, "vertex_colors", None)))


def cull_to_raster(mesh, t_wc, intrinsics, width, height, **kw):
    """``cull_mesh_faces`` by ``visible_faces`` (its arguments): the part of ``mesh`` that is nearest somewhere in some view."""
    return cull_mesh_faces(mesh, visible_faces(mesh, t_wc, intrinsics, width, height, **kw))


def compare_depth(a, b):
    """Two depth stacks [K, W, H] (a value > 0 is a measurement) compared pixel by pixel: a dict of per-view numpy arrays ``n_both``,
    ``n_a_only``, ``n_b_only``, ``sum_q`` (int64; the absolute differences of the pixels both measured, each quantised to 2^-20 m
    and summed as integers: exact, identical from run to run) and ``l1`` in metres (sum_q / 2^20 / n_both; NaN where n_both == 0)."""
    lib = _lib.load()
    dev = _device()
    a = torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous()
    b = torch.as_tensor(b).to(device=dev, dtype=torch.float32).contiguous()
    if a.dim() != 3 or a.shape != b.shape or a.numel() == 0:
        raise _lib.VmapStepError("compare_depth: two non-empty depth stacks [K, W, H] of one shape")
    K = int(a.shape[0])
    out = torch.empty((K, 4), dtype=torch.int64, device=dev)
    stream = _devmem.stream(dev)
    for k0 in range(0, K, 65535):
        k1 = min(K, k0 + 65535)
        _lib.check(lib.vmapstep_depth_compare(a[k0:k1].data_ptr(), b[k0:k1].data_ptr(), k1 - k0, int(a.shape[1] * a.shape[2]), out[k0:k1].data_ptr(), stream), lib)
    c = out.cpu().numpy()
    with np.errstate(all="ignore"):
        l1 = np.where(c[:, 0] > 0, c[:, 3] / 2.0 ** 20 / np.maximum(c[:, 0], 1), np.nan)
    return {"n_both": c[:, 0].copy(), "n_a_only": c[:, 1].copy(), "n_b_only": c[:, 2].copy(), "sum_q": c[:, 3].copy(), "l1": l1}


def depth_l1(rec, gt, t_wc, intrinsics, width, height, *, min_depth, max_depth=None, slots=None, budget_bytes=DEFAULT_BUDGET):
    """Depth L1 of a reconstruction against the ground truth from the poses ``t_wc``: both meshes rasterised, then ``compare_depth``
    (a = rec, b = gt) - its dict plus ``depth_l1``, the mean over all pixels both measured, all views together.  ``rec`` may equally
    be a depth stack [K, W, H] (``render.View.depth`` images of the trained fields, stacked), one image per drawn view."""
    kw = dict(min_depth=min_depth, max_depth=max_depth, slots=slots, budget_bytes=budget_bytes)
    b = rasterize(gt, t_wc, intrinsics, width, height, **kw).depth
    is_stack = isinstance(rec, (torch.Tensor, np.ndarray))
    a = torch.as_tensor(rec) if is_stack else rasterize(rec, t_wc, intrinsics, width, height, **kw).depth
    out = compare_depth(a, b)
    n = int(out["n_both"].sum())
    out["depth_l1"] = float(out["sum_q"].sum()) / 2.0 ** 20 / n if n else float("nan")
    return out
