"""Object bounds on the device: the reference's ``sceneObject.get_bound`` (vmap.py:270-315) without Open3D, trimesh or qhull.

``object_points``    every pixel of every keyframe of an object whose instance id is the object's and whose depth is > 0, unprojected
                     to the world (vmapstep_unproject_count / _emit, csrc/bounds_kernels.h), for a whole object list in one call:
                     one CSR-segmented float32 cloud ordered by (object, keyframe index, pixel index w * H + h).
``oriented_bounds``  a small-volume oriented box per segment, found by a search over orientations whose inner loop is the hot kernel
                     ``obb_extents`` (minimum / maximum of the points' projections on the axes of many candidate frames at once).
``get_bounds``       both; ``ObjectKeyframes.get_bound`` is the single-object form.

The search (shipped parameters, module constants below):
- the cloud is centred on the middle of its coordinate range (float32), which the unprojection's count pass already produced;
- round 0 evaluates one coarse set shared by all objects: first axis on a Fibonacci hemisphere of COARSE_DIRECTIONS = 1024
  directions, in-plane angle in COARSE_ANGLES = 16 steps over [0, 90 degrees): 16384 candidates, exactly 16 workgroups of candidates;
- each object keeps SEEDS = 8 frames: the best COARSE_SEEDS = 6 of the coarse set, the identity and the eigenvector frame of its
  covariance (so the result is never worse than the axis-aligned box or than ``evaluation.principal_axes_box``);
- ROUNDS = 6 refinement rounds: every seed is perturbed by the rotation vectors of a GRID^3 = 5 x 5 x 5 grid of radius delta (the
  seed itself is the grid's centre, so a seed's volume can only go down) and replaced by the best of its grid; delta starts at
  DELTA0_DEG = 2.8125 degrees (half the coarse in-plane step) and halves every round: the last round has delta = 0.0879 degrees
  and the final angular step is FINAL_STEP_DEG = 0.0439 degrees;
- the box is the best seed of the last round.
Per call the work is 1 + ROUNDS extents launches, one moments launch and two host reads (the moments, the result), whatever the
number of objects.  Candidates are generated in float64 and handed to the kernel as float32; the returned R is exactly the float32
frame the extents were measured in.

Box assembly (vmap.py:293-307): R has the box axes as columns (what ``meshing.bound_affine`` and the clip kernel expect) and
det R = +1; the extents are sorted ascending (nothing downstream depends on the order); centre = the middle of the projections'
range mapped back to the world; ``extent = max(extent, 0.10)`` as the reference does.  ``None`` where the reference returns None:
fewer than 4 points, or a cloud flat to rounding.

Deviations from the reference, all deliberate:
- a search over orientations instead of trimesh's enumeration of convex-hull faces (both are heuristics for the minimum-volume box;
  this one needs no hull and its inner loop is a pure min / max reduction);
- float32 points and projections (Open3D and trimesh work in float64);
- the flatness rule: smallest raw extent <= 2^-20 of the largest stands in for qhull's own coplanarity test.

The extents come from a backend: the HIP kernels for a device cloud, a small numpy implementation for a host cloud - the search
logic is the same code (torch on either device), so the CPU test tier runs it.
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import torch

from . import _devmem, _lib
from .meshing import BoundingBox

__all__ = ["object_points", "oriented_bounds", "get_bounds", "coarse_rotations", "extents",
           "COARSE_DIRECTIONS", "COARSE_ANGLES", "COARSE_SEEDS", "SEEDS", "ROUNDS", "GRID", "DELTA0_DEG", "FINAL_STEP_DEG", "MIN_EXTENT"]

COARSE_DIRECTIONS = 1024
COARSE_ANGLES = 16
COARSE_SEEDS = 6
SEEDS = COARSE_SEEDS + 2
ROUNDS = 6
GRID = 5
DELTA0_DEG = 90.0 / 32
FINAL_STEP_DEG = DELTA0_DEG / 2 ** (ROUNDS - 1) / ((GRID - 1) // 2)
MIN_EXTENT = 0.10
FLAT_RATIO = 2.0 ** -20


# ---- unprojection ----------------------------------------------------------------------------------------------------------------

def _intrinsics4(intrinsics):
    """(fx, fy, cx, cy) from a 4-sequence, a 3 x 3 matrix or anything with those four attributes."""
    if all(hasattr(intrinsics, k) for k in ("fx", "fy", "cx", "cy")):
        return tuple(float(getattr(intrinsics, k)) for k in ("fx", "fy", "cx", "cy"))
    a = np.asarray(intrinsics, np.float64)
    if a.shape == (3, 3):
        return float(a[0, 0]), float(a[1, 1]), float(a[0, 2]), float(a[1, 2])
    if a.shape == (4,):
        return tuple(float(v) for v in a)
    raise _lib.VmapStepError("intrinsics: (fx, fy, cx, cy), a 3 x 3 matrix or an object with fx, fy, cx, cy")


def _object_points(objects, intrinsics):
    """(points float32 [N, 3] on the store's device, host offsets int64 [n_obj + 1], bounds float32 [n_obj, 6] on the device)."""
    objects = list(objects)
    if not objects:
        raise _lib.VmapStepError("object_points: no objects")
    store = objects[0].store
    if any(o.store is not store for o in objects):
        raise _lib.VmapStepError("object_points: the objects must share one FrameStore")
    dev = store.device
    if dev.type != "cuda":
        raise _lib.VmapStepError("object_points runs on the GPU (no CPU fallback)")
    lib = _lib.load()
    pairs, first = [], [0]
    for o in objects:
        pairs += [(o.slots[k], o.obj_id) for k in range(o.n_keyframes) if o.slots[k] >= 0]
        first.append(len(pairs))
    n_obj, n_pairs = len(objects), len(pairs)
    first_h = np.asarray(first, np.int32)
    first_d = torch.from_numpy(first_h).to(dev)
    pairs_d = torch.tensor(pairs if pairs else [(0, 0)], dtype=torch.int32).reshape(-1, 2).to(dev)
    k4 = (ctypes.c_float * 4)(*_intrinsics4(intrinsics))
    depth, inst, t_wc = store.depth, store.inst, store.t_wc
    if not (depth.is_contiguous() and inst.is_contiguous() and t_wc.is_contiguous()):
        raise _lib.VmapStepError("object_points: the FrameStore tensors must be contiguous")
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_unproject_workspace_bytes, dev, n_pairs, n_obj, store.W, store.H)
    offsets = torch.empty(n_obj + 1, dtype=torch.int64, device=dev)
    bounds = torch.empty(n_obj, 6, dtype=torch.float32, device=dev)
    head = (depth.data_ptr(), inst.data_ptr(), t_wc.data_ptr(), store.capacity, store.W, store.H, k4, pairs_d.data_ptr(), first_d.data_ptr(),
            first_h.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n_obj, n_pairs)
    with torch.cuda.device(dev):
        stream = _devmem.stream(dev)
        _lib.check(lib.vmapstep_unproject_count(*head, offsets.data_ptr(), bounds.data_ptr(), ws_ptr, nbytes, stream), lib)
        off_h = offsets.cpu().numpy()               # the one host synchronisation
        n = int(off_h[-1])
        points = torch.empty(n, 3, dtype=torch.float32, device=dev)
        _lib.check(lib.vmapstep_unproject_emit(*head, points.data_ptr(), n, ws_ptr, nbytes, stream), lib)
    del ws
    return points, off_h, bounds


def object_points(objects, intrinsics):
    """The clouds of ``objects`` (``ObjectKeyframes`` over one ``FrameStore``): (points float32 [N, 3] on the device, offsets int64
    [n_obj + 1] on the host).  Object o owns points[offsets[o]:offsets[o + 1]], ordered by keyframe index, then pixel index."""
    points, offsets, _ = _object_points(objects, intrinsics)
    return points, offsets


# ---- candidate frames -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _coarse(m_dirs, n_angles):
    m = np.arange(m_dirs, dtype=np.float64)
    z = (m + 0.5) / m_dirs                                   # the upper hemisphere: a box axis and its negative are one candidate
    phi = m * (math.pi * (3.0 - math.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    a = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)
    helper = np.zeros_like(a)
    helper[np.arange(m_dirs), np.argmin(np.abs(a), 1)] = 1.0
    b0 = np.cross(a, helper)
    b0 /= np.linalg.norm(b0, axis=1, keepdims=True)
    c0 = np.cross(a, b0)
    psi = np.arange(n_angles, dtype=np.float64) * (0.5 * math.pi / n_angles)
    b = np.cos(psi)[None, :, None] * b0[:, None, :] + np.sin(psi)[None, :, None] * c0[:, None, :]
    aa = np.broadcast_to(a[:, None, :], b.shape)
    c = np.cross(aa, b)
    R = np.stack([aa, b, c], 2).reshape(-1, 3, 3)
    R.setflags(write=False)
    return R


def coarse_rotations():
    """The shared coarse set: float64 [COARSE_DIRECTIONS * COARSE_ANGLES, 3, 3], rows = box axes, det = +1."""
    return _coarse(COARSE_DIRECTIONS, COARSE_ANGLES)


def _grid_vectors(device):
    t = torch.linspace(-1.0, 1.0, GRID, dtype=torch.float64, device=device)
    return torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)


def _exp_so3(w):
    """Rodrigues: [..., 3] rotation vectors -> [..., 3, 3]; the zero vector gives the identity exactly."""
    th2 = (w * w).sum(-1)
    th = th2.sqrt()
    small = th < 1e-12
    ths = torch.where(small, torch.ones_like(th), th)
    A = torch.where(small, torch.ones_like(th), torch.sin(ths) / ths)
    B = torch.where(small, torch.full_like(th, 0.5), (1.0 - torch.cos(ths)) / (ths * ths))
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    zero = torch.zeros_like(x)
    Kx = torch.stack([torch.stack([zero, -z, y], -1), torch.stack([z, zero, -x], -1), torch.stack([-y, x, zero], -1)], -2)
    K2 = _mul3(Kx, Kx)
    eye = torch.eye(3, dtype=w.dtype, device=w.device).expand_as(Kx)
    return eye + A[..., None, None] * Kx + B[..., None, None] * K2


def _mul3(a, b):
    """a @ b for [..., 3, 3] written out elementwise: the rounding of an entry does not depend on the batch it is in."""
    return a[..., :, 0:1] * b[..., 0:1, :] + a[..., :, 1:2] * b[..., 1:2, :] + a[..., :, 2:3] * b[..., 2:3, :]


# ---- extents backends -------------------------------------------------------------------------------------------------------------

class _HipBackend:
    """The extents of a device cloud from vmapstep_obb_extents; the moments from vmapstep_cloud_moments."""

    def __init__(self, points, offsets_host, point_chunks=0):
        self.lib = _lib.load()
        self.dev = points.device
        self.points = points
        self.off_h = np.ascontiguousarray(offsets_host, np.int64)
        self.off_d = torch.from_numpy(self.off_h).to(self.dev)
        self.n_obj = len(self.off_h) - 1
        self.point_chunks = int(point_chunks)

    def _off_p(self):
        return self.off_h.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def extents(self, rotations, center=None):
        """rotations float32 [K, 3, 3] (shared) or [n_obj, K, 3, 3] on the device -> lo, hi float32 [n_obj, K, 3]."""
        rot = rotations.to(device=self.dev, dtype=torch.float32).contiguous()
        shared = rot.dim() == 3
        K = rot.shape[0] if shared else rot.shape[1]
        lo = torch.empty(self.n_obj, K, 3, dtype=torch.float32, device=self.dev)
        hi = torch.empty_like(lo)
        c = None if center is None else center.to(device=self.dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.vmapstep_obb_extents(self.points.data_ptr(), len(self.points), self.off_d.data_ptr(), self._off_p(), self.n_obj,
                                                     None if c is None else c.data_ptr(), rot.data_ptr(), 0 if shared else 9 * K, K,
                                                     self.point_chunks, lo.data_ptr(), hi.data_ptr(), _devmem.stream(self.dev)), self.lib)
        return lo, hi

    def moments(self, center):
        c = center.to(device=self.dev, dtype=torch.float32).contiguous()
        out = torch.empty(self.n_obj, 9, dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.vmapstep_cloud_moments(self.points.data_ptr(), len(self.points), self.off_d.data_ptr(), self._off_p(), self.n_obj,
                                                       c.data_ptr(), out.data_ptr(), _devmem.stream(self.dev)), self.lib)
        return out.cpu().numpy()


class _NumpyBackend:
    """The same two functions on the host (float32 projections by matrix product): for the CPU test tier and for comparison."""
    CHUNK = 2048                                             # candidates per matrix product

    def __init__(self, points, offsets_host, point_chunks=0):
        self.dev = torch.device("cpu")
        self.points = np.ascontiguousarray(points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points, np.float32).reshape(-1, 3)
        self.off_h = np.ascontiguousarray(offsets_host, np.int64)
        self.n_obj = len(self.off_h) - 1

    def _centred(self, o, center):
        p = self.points[self.off_h[o]:self.off_h[o + 1]]
        return p if center is None else p - center[o]

    def extents(self, rotations, center=None):
        rot = rotations.detach().cpu().numpy().astype(np.float32)
        c = None if center is None else center.detach().cpu().numpy().astype(np.float32)
        shared = rot.ndim == 3
        K = rot.shape[0] if shared else rot.shape[1]
        lo = np.full((self.n_obj, K, 3), np.inf, np.float32)
        hi = np.full((self.n_obj, K, 3), -np.inf, np.float32)
        for o in range(self.n_obj):
            q = self._centred(o, c)
            if len(q) == 0:
                continue
            r = rot if shared else rot[o]
            for k0 in range(0, K, self.CHUNK):
                proj = q @ r[k0:k0 + self.CHUNK].reshape(-1, 3).T                    # [n, 3 * chunk]
                lo[o, k0:k0 + self.CHUNK] = proj.min(0).reshape(-1, 3)
                hi[o, k0:k0 + self.CHUNK] = proj.max(0).reshape(-1, 3)
        return torch.from_numpy(lo), torch.from_numpy(hi)

    def moments(self, center):
        c = center.detach().cpu().numpy().astype(np.float32)
        out = np.zeros((self.n_obj, 9), np.float64)
        for o in range(self.n_obj):
            q = self.points[self.off_h[o]:self.off_h[o + 1]].astype(np.float64) - c[o].astype(np.float64)
            out[o, :3] = q.sum(0)
            out[o, 3:] = (q.T @ q)[np.triu_indices(3)]
        return out


_BACKENDS = {"hip": _HipBackend, "numpy": _NumpyBackend}


def _backend(points, offsets, backend, point_chunks=0):
    if offsets is None:
        offsets = [0, len(points)]
    off_h = np.asarray(offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, np.int64).reshape(-1)
    if len(off_h) < 2 or off_h[0] < 0 or np.any(np.diff(off_h) < 0) or off_h[-1] > len(points):
        raise _lib.VmapStepError("oriented_bounds: offsets must be non-decreasing inside [0, len(points)]")
    if backend is None:
        backend = "hip" if isinstance(points, torch.Tensor) and points.device.type == "cuda" else "numpy"
    if backend == "hip":
        if not (isinstance(points, torch.Tensor) and points.device.type == "cuda"):
            if not torch.cuda.is_available():
                raise _lib.VmapStepError("oriented_bounds(backend='hip') runs on the GPU")
            points = torch.as_tensor(np.asarray(points, np.float32) if not isinstance(points, torch.Tensor) else points).to("cuda")
        points = points.to(torch.float32).reshape(-1, 3).contiguous()
    elif backend != "numpy":
        raise _lib.VmapStepError(f"oriented_bounds: unknown backend {backend!r}")
    return _BACKENDS[backend](points, off_h, point_chunks)


def extents(points, rotations, offsets=None, center=None, backend=None, point_chunks=0):
    """lo, hi float32 [n_obj, K, 3]: the range of every segment's points (minus ``center`` [n_obj, 3], if given) projected on the rows
    of ``rotations`` ([K, 3, 3] shared by all segments, or [n_obj, K, 3, 3]).  ``point_chunks``: the hip backend's launch geometry
    (workgroups per object along the points; 0 = automatic) - the result does not depend on it."""
    be = _backend(points, offsets, backend, point_chunks)
    rot = torch.as_tensor(rotations).to(be.dev)
    c = None if center is None else torch.as_tensor(center).to(be.dev)
    return be.extents(rot, c)


# ---- the search -------------------------------------------------------------------------------------------------------------------

def _volume(lo, hi):
    e = (hi - lo).double()
    return e[..., 0] * e[..., 1] * e[..., 2]


def _covariance_frames(moments, counts):
    """Rows = eigenvectors of each covariance, largest eigenvalue first, right-handed (principal_axes_box's frame).  Per object on the
    host, so that an object's frame does not depend on the batch."""
    out = np.zeros((len(counts), 3, 3))
    for o, n in enumerate(counts):
        n = max(int(n), 1)
        mu = moments[o, :3] / n
        S = np.zeros((3, 3))
        S[np.triu_indices(3)] = moments[o, 3:] / n
        S = S + S.T - np.diag(np.diag(S)) - np.outer(mu, mu)
        if not np.all(np.isfinite(S)):
            S = np.eye(3)
        _, vec = np.linalg.eigh(S)
        R = vec[:, ::-1].T.copy()
        if np.linalg.det(R) < 0:
            R[2] = -R[2]
        out[o] = R
    return out


def _search(be, bounds=None):
    """-> per object: R32 [3, 3] (rows = axes), lo, hi [3], centre c0 [3] (host arrays) and the volumes (coarse best, final)."""
    dev, n_obj = be.dev, be.n_obj
    if bounds is None:
        lo0, hi0 = be.extents(torch.eye(3, dtype=torch.float32, device=dev)[None])
        lo0, hi0 = lo0[:, 0], hi0[:, 0]
    else:
        lo0, hi0 = bounds[:, :3].to(dev), bounds[:, 3:].to(dev)
    c0 = 0.5 * lo0 + 0.5 * hi0
    c0 = torch.where(torch.isfinite(c0), c0, torch.zeros_like(c0)).to(torch.float32)           # an empty cloud: (+inf - inf)
    counts = np.diff(be.off_h)
    pca = torch.from_numpy(_covariance_frames(be.moments(c0), counts)).to(dev)                 # host read 1 of 2

    coarse = torch.from_numpy(np.array(coarse_rotations())).to(dev)
    lo, hi = be.extents(coarse.to(torch.float32), c0)
    vol = _volume(lo, hi)
    vol = torch.where(torch.isnan(vol), torch.full_like(vol, math.inf), vol)
    coarse_best = vol.min(1).values
    picks = []
    for _ in range(COARSE_SEEDS):
        idx = vol.argmin(1)
        picks.append(idx)
        vol = vol.scatter(1, idx[:, None], math.inf)
    seeds = torch.cat([coarse[torch.stack(picks, 1)],                                          # [n_obj, COARSE_SEEDS, 3, 3]
                       torch.eye(3, dtype=torch.float64, device=dev).expand(n_obj, 1, 3, 3), pca[:, None]], 1)
    grid = _grid_vectors(dev)
    G = len(grid)
    delta = math.radians(DELTA0_DEG)
    rows = torch.arange(n_obj, device=dev)[:, None]
    for _ in range(ROUNDS):
        cand = _mul3(_exp_so3(grid * delta)[None, None], seeds[:, :, None])                   # [n_obj, SEEDS, G, 3, 3]
        cand32 = cand.to(torch.float32)
        lo, hi = be.extents(cand32.reshape(n_obj, SEEDS * G, 3, 3), c0)
        vol = _volume(lo, hi).reshape(n_obj, SEEDS, G)
        vol = torch.where(torch.isnan(vol), torch.full_like(vol, math.inf), vol)
        best = vol.argmin(2)                                                                   # [n_obj, SEEDS]
        seeds = cand[rows, torch.arange(SEEDS, device=dev)[None], best]
        delta *= 0.5
    seed_vol = vol.gather(2, best[..., None])[..., 0]
    s = seed_vol.argmin(1)
    k = s * G + best[rows[:, 0], s]
    o = rows[:, 0]
    pack = torch.cat([cand32.reshape(n_obj, SEEDS * G, 9)[o, k].double(), lo[o, k].double(), hi[o, k].double(), c0.double(),
                      coarse_best[:, None], seed_vol[o, s][:, None]], 1).cpu().numpy()        # host read 2 of 2
    return pack


def _assemble(row, n_points, min_extent=MIN_EXTENT):
    """One BoundingBox (or None) from a result row of _search."""
    if n_points < 4:
        return None
    R32, lo, hi, c0 = row[:9].reshape(3, 3), row[9:12], row[12:15], row[15:18]
    raw = hi - lo
    if not np.all(np.isfinite(raw)) or raw.min() <= FLAT_RATIO * raw.max():
        return None
    order = np.argsort(raw, kind="stable")
    axes = R32[order]
    centre = c0 + (0.5 * (lo + hi)) @ R32
    R = axes.T.copy()
    if np.linalg.det(R) < 0:
        R[:, 2] = -R[:, 2]
    return BoundingBox(center=centre, R=R, extent=np.maximum(raw[order], min_extent))


def oriented_bounds(points, offsets=None, backend=None, bounds=None, return_info=False, min_extent=MIN_EXTENT):
    """A small-volume oriented box of every segment of ``points`` ([N, 3]; ``offsets`` [n + 1], default one segment) as a list of
    ``BoundingBox`` (centre, R with the box axes as columns, full extents ascending and >= MIN_EXTENT) or ``None`` (fewer than 4
    points, or flat to rounding).  ``backend``: 'hip' (default for a device tensor) or 'numpy' (default otherwise).  ``bounds``
    [n, 6] float32: the coordinate minimum and maximum of every segment if already known (saves one pass).  ``min_extent``: the
    floor of every extent (the reference's 0.10; 0.0 leaves the found box as it is).  With ``return_info``
    also a dict of per-segment arrays: 'coarse_volume' (the best of the coarse set), 'volume' (the found box before clamping)."""
    be = _backend(points, offsets, backend)
    pack = _search(be, None if bounds is None else torch.as_tensor(bounds, dtype=torch.float32))
    counts = np.diff(be.off_h)
    boxes = [_assemble(pack[o], int(counts[o]), float(min_extent)) for o in range(be.n_obj)]
    if return_info:
        return boxes, {"coarse_volume": pack[:, 18].copy(), "volume": pack[:, 19].copy()}
    return boxes


def get_bounds(objects, intrinsics):
    """``sceneObject.get_bound`` for a list of ``ObjectKeyframes`` over one ``FrameStore``: one ``BoundingBox`` or ``None`` each."""
    points, offsets, bounds = _object_points(objects, intrinsics)
    return oriented_bounds(points, offsets, backend="hip", bounds=bounds)
