"""Visibility culling on the device: keep what the keyframes saw of a mesh.

A field extracted through ``Trainer.meshing`` is closed everywhere inside its box - the back of a sofa, the underside of a table -
and none of that was observed.  Scene-level evaluation therefore first removes what no frame saw, from the reconstruction and from
the ground truth, and scores the rest.  ``mark_visible`` asks "was this point seen?" of every point of a cloud against a set of
frames (depth images and poses, a ``FrameStore`` in place), ``cull_mesh`` compacts a mesh by such a mask.  The rule is
csrc/cull_rules.h's, the kernels csrc/cull_kernels.h's, the contract the cull section of include/vmapstep.h; it is this project's
own - the reference leaves the step to outside tools.

The known limit: a face is judged by its corners.  A large triangle whose corners all miss every frustum is dropped even if its
middle was seen (coarse ground-truth meshes have such triangles).  The remedy is to cull samples, not vertices: draw the points with
``evaluation.sample_surface`` and pass them to ``mark_visible`` - or to cull by what won a pixel: ``raster.cull_to_raster`` keeps
exactly the faces that are nearest somewhere in some view."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _devmem, _lib
from .bounds import _intrinsics4
from .meshing import Mesh

__all__ = ["mark_visible", "mark_visible_store", "cull_mesh", "cull_to_views"]


def _device():
    if not torch.cuda.is_available():
        raise _lib.VmapStepError("visibility culling runs on the GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _slots(slots, n_slots, device):
    """(device int32 tensor or None, frames): ``slots`` checked on the host - the library cannot check device values."""
    if slots is None:
        return None, n_slots
    host = (slots.detach().cpu().numpy() if isinstance(slots, torch.Tensor) else np.asarray(slots)).astype(np.int64).reshape(-1)
    if len(host) and (host.min() < 0 or host.max() >= n_slots):
        raise _lib.VmapStepError(f"slots must lie in [0, {n_slots})")
    return torch.from_numpy(host.astype(np.int32)).to(device), len(host)


def mark_visible(points, depth, t_wc, intrinsics, occlusion_eps, *, seen=None, slots=None, margin=0, min_depth=0.0, size=None):
    """Which of ``points`` ([n, 3], numpy or tensor) any of the frames saw, as a uint8 device tensor [n] (1 = seen).

    ``depth`` [K, W, H] float32 (width-major, as a ``FrameStore`` holds it) and ``t_wc`` [K, 4, 4] camera-to-world poses (rotations
    assumed orthonormal); ``intrinsics``: (fx, fy, cx, cy), a 3 x 3 matrix or an object with those attributes.  ``occlusion_eps`` is
    required: a tolerance in metres - a point is seen by a frame iff it projects (rounded half to even) onto a pixel inside the image
    less ``margin``, lies farther than ``min_depth`` along the optical axis and not more than ``occlusion_eps`` behind the depth
    measured there - or ``None`` for the frustum test alone; then ``depth`` may be ``None`` with ``size=(width, height)``.
    ``slots``: the frames to use, as indices into ``depth`` / ``t_wc`` (default: all, in order).  ``seen``: a mask from an earlier
    call to add to - the call only ever turns a 0 into a 1, so frames may be marked in chunks.

    ``points`` is any cloud.  Mesh vertices are the main use; surface samples from ``evaluation.sample_surface`` are the other: a
    sample has no extent, which avoids the large-triangle problem of coarse ground-truth meshes (see the module's docstring)."""
    lib = _lib.load()
    dev = _device()
    p = (points if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points)))
    p = p.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    poses = torch.as_tensor(t_wc).to(device=dev, dtype=torch.float32).reshape(-1, 4, 4).contiguous()
    if depth is None:
        if occlusion_eps is not None:
            raise _lib.VmapStepError("mark_visible: occlusion_eps needs depth images (pass occlusion_eps=None for the frustum test alone)")
        if size is None:
            raise _lib.VmapStepError("mark_visible: without depth images pass size=(width, height)")
        width, height = int(size[0]), int(size[1])
        d = None
    else:
        d = torch.as_tensor(depth).to(device=dev, dtype=torch.float32)
        if d.dim() != 3 or d.shape[0] != poses.shape[0]:
            raise _lib.VmapStepError("mark_visible: depth [K, W, H] and t_wc [K, 4, 4]")
        d = d.contiguous()
        width, height = int(d.shape[1]), int(d.shape[2])
        if size is not None and (int(size[0]), int(size[1])) != (width, height):
            raise _lib.VmapStepError("mark_visible: size differs from the depth images'")
    sl, n_frames = _slots(slots, int(poses.shape[0]), dev)
    if seen is None:
        seen = torch.zeros(len(p), dtype=torch.uint8, device=dev)
    elif not (isinstance(seen, torch.Tensor) and seen.dtype == torch.uint8 and seen.device == dev and seen.is_contiguous() and seen.numel() == len(p)):
        raise _lib.VmapStepError("mark_visible: seen must be a contiguous uint8 tensor [n] on the device")
    if n_frames == 0 or len(p) == 0:
        return seen
    fx, fy, cx, cy = _intrinsics4(intrinsics)
    use_depth = occlusion_eps is not None
    cfg = _lib.CullCfg(fx, fy, cx, cy, float(min_depth), float(occlusion_eps) if use_depth else 0.0, width, height, int(margin), int(use_depth))
    _lib.check(lib.vmapstep_cull_mark(p.data_ptr(), len(p), d.data_ptr() if use_depth else None, poses.data_ptr(),
                                      None if sl is None else sl.data_ptr(), n_frames, ctypes.byref(cfg), seen.data_ptr(), _devmem.stream(dev)), lib)
    return seen


def mark_visible_store(points, store, intrinsics, occlusion_eps, slots=None, **kw):
    """``mark_visible`` over the frames of a ``FrameStore``, read in place (no copy of its depth images or poses).  ``slots``
    defaults to every slot that holds a frame (``frame_of_slot`` is not ``None``)."""
    if slots is None:
        slots = [s for s, f in enumerate(store.frame_of_slot) if f is not None]
    with torch.cuda.device(store.device):
        return mark_visible(points, store.depth, store.t_wc, intrinsics, occlusion_eps, slots=slots, **kw)


def cull_mesh(mesh, seen, min_seen=1):
    """The part of ``mesh`` the mask keeps, as a ``Mesh``, or ``None`` when no face is left.  A face is kept iff at least ``min_seen``
    (1, 2 or 3) of its corners are seen; a vertex iff a kept face references it (with ``min_seen`` < 3 that includes unseen corners).
    Faces keep their order, vertices their ascending order; normals and colours travel with their vertices.  One host
    synchronisation, for the two counts."""
    lib = _lib.load()
    dev = _device()
    v = torch.as_tensor(mesh.vertices).to(device=dev, dtype=torch.float32).reshape(-1, 3)
    f = torch.as_tensor(mesh.faces).to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    s = torch.as_tensor(seen).to(device=dev)
    s = (s != 0).to(torch.uint8).contiguous() if s.dtype != torch.uint8 else s.contiguous()
    if s.numel() != len(v):
        raise _lib.VmapStepError("cull_mesh: one mask entry per vertex")
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_cull_workspace_bytes, dev, len(v), len(f))
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    stream = _devmem.stream(dev)
    _lib.check(lib.vmapstep_cull_faces_count(f.data_ptr(), len(f), s.data_ptr(), len(v), int(min_seen), counts.data_ptr(), ws_ptr, nbytes, stream), lib)
    nf, nv = (int(x) for x in counts.cpu())            # the one host synchronisation
    if nf == 0:
        return None
    kept = torch.empty(nv, dtype=torch.int32, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    _lib.check(lib.vmapstep_cull_faces_emit(f.data_ptr(), len(f), s.data_ptr(), len(v), int(min_seen), kept.data_ptr(), nv, faces.data_ptr(), nf,
                                            ws_ptr, nbytes, stream), lib)
    del ws
    idx = kept.long()
    gather = lambda t: None if t is None else torch.as_tensor(t).to(dev)[idx]
    return Mesh(v[idx], faces, gather(getattr(mesh, "vertex_normals", None)), gather(getattr(mesh, "vertex_colors", None)))


def cull_to_views(mesh, depth, t_wc, intrinsics, occlusion_eps, min_seen=1, **kw):
    """``cull_mesh`` by what the frames saw of the mesh's vertices (``mark_visible``'s arguments; ``kw`` goes to it)."""
    return cull_mesh(mesh, mark_visible(mesh.vertices, depth, t_wc, intrinsics, occlusion_eps, **kw), min_seen)
