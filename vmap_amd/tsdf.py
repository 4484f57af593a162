"""TSDF fusion on the device: posed depth keyframes, for the whole scene or masked to one object, fused into a truncated signed distance
volume and meshed - the TSDF-Fusion baseline the paper compares its object fields against, a model for ``DepthTracker.track_to_mesh``
before any field has converged, and a mesh seconds after ingest.  The rule is csrc/tsdf_rules.h's, the kernel csrc/tsdf_kernels.h's,
the contract the tsdf section of include/vmapstep.h; it is this project's own - no outside library is involved.

A volume is three device tensors: ``tsdf`` and ``weight`` float32 [nx, ny, nz] and, with ``color=True``, ``color`` float32
[nx*ny*nz, 4] (r, g, b on the 0..255 scale and the colour's own weight).  The TSDF is in units of ``trunc``, in [-1, 1], negative
inside; a voxel no frame has updated has weight 0 and yields no surface.  Frames are taken in batches: the volume is read and written
once per ``integrate`` call, whatever the number of frames, and the result depends on the order of the frames alone - one call over K
frames equals two calls over its halves bit for bit.

``TSDFVolume.raycast`` reads a volume out directly as depth, status, normal and colour images from any poses, with no mesh in between
(csrc/raycast_rules.h, csrc/raycast_kernels.h, the raycast section of include/vmapstep.h): the model image of
``DepthTracker.track_to_volume``, and a volume-side input of ``raster.compare_depth``.

    python -m vmap_amd.tsdf FRAMES.npz OUT.ply --voxel-size X --trunc Y [--obj-id N] [--views OUT.npz]

reads depth [K,W,H], t_wc [K,4,4], intrinsics [4] (the file ``python -m vmap_amd.evaluation --frames`` reads) and optionally rgb
[K,W,H,3] uint8 and inst [K,W,H] integers.  ``--views`` also writes the ray cast of the fused volume at the frames' own poses: depth,
status, normal, t_wc and, with rgb, color."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _devmem, _lib
from .bounds import _intrinsics4
from .meshing import BoundingBox, bound_affine, extract_mesh
from .visibility import _device, _slots

__all__ = ["TSDFVolume", "VolumeView", "fuse_object"]

FLT_MAX = float(np.finfo(np.float32).max)      # the default max_depth: every finite depth counts, inf does not


class VolumeView:
    """What ``TSDFVolume.raycast`` returns, on the volume's device: ``depth`` float32 [K, W, H] (0 = no hit), ``status`` uint8 [K, W, H]
    (``MISS`` the volume or the depth range, ``HIT``, ``LEFT`` the range without a crossing, ended ``BEHIND`` a surface, ran out of
    ``STEPS``), ``normal`` float32 [K, W, H, 3] or None (world frame, unit length, to free space; zero where refused), ``color`` uint8
    [K, W, H, 4] or None, and ``t_wc`` float32 [K, 4, 4] on the host: the float32 poses the images were actually cast from."""
    MISS, HIT, LEFT, BEHIND, STEPS = _lib.RAYCAST_MISS, _lib.RAYCAST_HIT, _lib.RAYCAST_LEFT, _lib.RAYCAST_BEHIND, _lib.RAYCAST_STEPS

    def __init__(self, depth, status, normal, color, t_wc):
        self.depth, self.status, self.normal, self.color, self.t_wc = depth, status, normal, color, t_wc


class TSDFVolume:
    def __init__(self, shape, affine, trunc, *, color=False, max_weight=64.0, device=None):
        """``shape``: (nx, ny, nz), each side 2..1024; ``affine``: [3,4], voxel index -> world (rows [A | b]); ``trunc`` in metres."""
        self.shape = tuple(int(s) for s in shape)
        if len(self.shape) != 3:
            raise _lib.VmapStepError("TSDFVolume: shape is (nx, ny, nz)")
        self.affine = np.asarray(affine, np.float64).reshape(3, 4).copy()
        self.trunc, self.max_weight = float(trunc), float(max_weight)
        if not self.trunc > 0 or not self.max_weight >= 1:
            raise _lib.VmapStepError("TSDFVolume: trunc > 0 and max_weight >= 1")
        self.device = _device() if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise _lib.VmapStepError("TSDF fusion runs on the GPU (no CPU fallback)")
        n = self.shape[0] * self.shape[1] * self.shape[2]
        self.tsdf = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        self.color = torch.zeros(n, 4, dtype=torch.float32, device=self.device) if color else None

    @classmethod
    def from_bound(cls, bound, *, voxel_size=None, grid_dim=None, trunc, **kw):
        """The volume of a ``meshing.BoundingBox`` (centre, R, full extent; oriented boxes welcome).  ``grid_dim``: that many voxels
        along every axis, the outermost centres on the box's faces - ``bound_affine``'s grid, the one ``Trainer.meshing`` queries.
        ``voxel_size``: cubic voxels of that edge, as many per axis as cover the extent (at least 2), centred on the box."""
        if (voxel_size is None) == (grid_dim is None):
            raise _lib.VmapStepError("from_bound: give voxel_size or grid_dim")
        if grid_dim is not None:
            return cls((int(grid_dim),) * 3, bound_affine(bound, 1.0, int(grid_dim)), trunc, **kw)
        ext = np.asarray(bound.extent, np.float64).reshape(3)
        dims = np.maximum(np.ceil(ext / float(voxel_size) - 1e-9).astype(np.int64) + 1, 2)
        R = np.asarray(bound.R, np.float64).reshape(3, 3)
        A = R * float(voxel_size)
        b = np.asarray(bound.center, np.float64).reshape(3) - A @ ((dims - 1) / 2.0)
        return cls(tuple(int(d) for d in dims), np.concatenate([A, b[:, None]], 1), trunc, **kw)

    def reset(self):
        self.tsdf.zero_()
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def integrate(self, depth, t_wc, intrinsics, *, rgb=None, inst=None, obj_id=None, slots=None, margin=0, min_depth=0.0, max_depth=FLT_MAX):
        """Fuse frames into the volume, in the order given.  ``depth`` [K, W, H] float32 (width-major, as a ``FrameStore`` holds it),
        ``t_wc`` [K, 4, 4] camera-to-world poses, ``intrinsics`` as ``visibility.mark_visible`` takes them; ``slots``: the frames to
        use and their order, as indices into ``depth`` / ``t_wc`` (default: all, in order; checked on the host).  ``rgb``: uint8
        [K, W, H, 3] or [K, W, H, 4] (a ``FrameStore``'s rgbx, read in place), required by a colour volume.  ``obj_id`` (with ``inst``
        int32 [K, W, H]): only pixels of that instance count.  A measurement d counts iff ``min_depth`` < d <= ``max_depth``."""
        lib = _lib.load()
        dev = self.device
        d = torch.as_tensor(depth).to(device=dev, dtype=torch.float32)
        poses = torch.as_tensor(t_wc).to(device=dev, dtype=torch.float32).reshape(-1, 4, 4).contiguous()
        if d.dim() != 3 or d.shape[0] != poses.shape[0]:
            raise _lib.VmapStepError("integrate: depth [K, W, H] and t_wc [K, 4, 4]")
        d = d.contiguous()
        K, width, height = (int(s) for s in d.shape)
        sl, n_frames = _slots(slots, K, dev)
        px = None
        if self.color is not None:
            if rgb is None:
                raise _lib.VmapStepError("integrate: a colour volume needs rgb")
            px = torch.as_tensor(rgb).to(device=dev)
            if px.dtype != torch.uint8 or px.dim() != 4 or tuple(px.shape[:3]) != (K, width, height) or px.shape[3] not in (3, 4):
                raise _lib.VmapStepError("integrate: rgb is uint8 [K, W, H, 3] or [K, W, H, 4]")
            if px.shape[3] == 3:
                px = torch.cat([px, torch.zeros_like(px[..., :1])], -1)
            px = px.contiguous()
        oid, ins = -1, None
        if obj_id is not None and int(obj_id) >= 0:
            if inst is None:
                raise _lib.VmapStepError("integrate: obj_id needs inst")
            ins = torch.as_tensor(inst).to(device=dev, dtype=torch.int32)
            if tuple(ins.shape) != (K, width, height):
                raise _lib.VmapStepError("integrate: inst [K, W, H]")
            ins, oid = ins.contiguous(), int(obj_id)
        if n_frames == 0:
            return self
        fx, fy, cx, cy = _intrinsics4(intrinsics)
        aff = (ctypes.c_float * 12)(*np.ascontiguousarray(self.affine, np.float32).reshape(-1).tolist())
        cfg = _lib.TsdfCfg(*self.shape, oid, aff, fx, fy, cx, cy, width, height, int(margin), 0, float(min_depth), float(max_depth),
                           self.trunc, self.max_weight)
        with torch.cuda.device(dev):
            _lib.check(lib.vmapstep_tsdf_integrate(ctypes.byref(cfg), self.tsdf.data_ptr(), self.weight.data_ptr(),
                                                   None if self.color is None else self.color.data_ptr(), d.data_ptr(),
                                                   None if px is None else px.data_ptr(), None if ins is None else ins.data_ptr(),
                                                   poses.data_ptr(), None if sl is None else sl.data_ptr(), n_frames, _devmem.stream(dev)), lib)
        return self

    def integrate_store(self, store, intrinsics, slots=None, obj_id=None, **kw):
        """``integrate`` over the frames of a ``FrameStore``, read in place.  ``slots`` defaults to every slot that holds a frame."""
        if slots is None:
            slots = [s for s, f in enumerate(store.frame_of_slot) if f is not None]
        return self.integrate(store.depth, store.t_wc, intrinsics, rgb=store.rgbx if self.color is not None else None,
                              inst=store.inst if obj_id is not None else None, obj_id=obj_id, slots=slots, **kw)

    def raycast(self, t_wc, intrinsics, width, height, *, min_depth, max_depth, min_weight=1.0, step=None, max_steps=4096, normals=True,
                color=None, use_bricks=True, library=None):
        """Depth, status, normal and colour images of the volume from the poses ``t_wc`` [K, 4, 4] (camera to world; a single [4, 4] is
        K = 1; an all-zero pose is an unused slot whose pixels all miss) -> ``VolumeView``.  A ray is cast over ``min_depth`` <= z <=
        ``max_depth`` in samples ``step`` metres apart along the ray (default ``trunc / 2``), at most ``max_steps`` of them, and hits where
        the TSDF, trilinear over voxels of weight >= ``min_weight``, first goes from > 0 to <= 0.  ``color``: default, whether the volume
        has colour.  The brick classes (exact empty-space skipping) are rebuilt on every call - one read of the volume, amortised over
        the K views; nothing is cached, ``tsdf`` and ``weight`` being public tensors.  ``use_bricks=False`` marches without them and
        gives the same bits.  ``library``: another build of the library (the measurement build of tests/tools)."""
        lib = _lib.load(library)
        dev = self.device
        poses = np.asarray(t_wc.detach().cpu().numpy() if isinstance(t_wc, torch.Tensor) else t_wc, np.float64)
        if poses.shape == (4, 4):
            poses = poses[None]
        if poses.ndim != 3 or poses.shape[1:] != (4, 4):
            raise _lib.VmapStepError("raycast: t_wc [K, 4, 4]")
        color = self.color is not None if color is None else bool(color)
        if color and self.color is None:
            raise _lib.VmapStepError("raycast: color=True needs a colour volume")
        step = self.trunc / 2 if step is None else float(step)
        width, height, K = int(width), int(height), len(poses)
        # the float32 rounding of the poses is what the images are cast from; M = A^-1 T_wc in float64, rounded once
        t32 = poses.astype(np.float32)
        A4 = np.eye(4)
        A4[:3] = self.affine
        A_inv = np.linalg.inv(A4)
        M = np.zeros((K, 12), np.float64)
        for k in range(K):
            if t32[k, :3].any():
                M[k] = (A_inv @ t32[k].astype(np.float64))[:3].reshape(12)
        nmap = (ctypes.c_float * 9)(*np.linalg.inv(self.affine[:, :3]).T.astype(np.float32).reshape(-1).tolist())
        fx, fy, cx, cy = _intrinsics4(intrinsics)
        cfg = _lib.RaycastCfg(*self.shape, width, height, int(max_steps), 0 if use_bricks else _lib.RAYCAST_IGNORE_BRICKS, 0, fx, fy, cx, cy,
                              float(min_depth), float(max_depth), step, float(min_weight), nmap, 0.0)
        with torch.cuda.device(dev):
            views = torch.from_numpy(M.astype(np.float32)).to(dev)
            depth = torch.empty((K, width, height), dtype=torch.float32, device=dev)
            status = torch.empty((K, width, height), dtype=torch.uint8, device=dev)
            normal = torch.empty((K, width, height, 3), dtype=torch.float32, device=dev) if normals else None
            col = torch.empty((K, width, height, 4), dtype=torch.uint8, device=dev) if color else None
            stream = _devmem.stream(dev)
            bricks = None
            if use_bricks and K:
                nb = ctypes.c_size_t()
                _lib.check(lib.vmapstep_tsdf_bricks_bytes(*self.shape, ctypes.byref(nb)), lib)
                bricks = torch.empty(nb.value, dtype=torch.uint8, device=dev)
                _lib.check(lib.vmapstep_tsdf_bricks(*self.shape, float(min_weight), self.tsdf.data_ptr(), self.weight.data_ptr(),
                                                    bricks.data_ptr(), stream), lib)
            _lib.check(lib.vmapstep_tsdf_raycast(ctypes.byref(cfg), self.tsdf.data_ptr(), self.weight.data_ptr(),
                                                 None if self.color is None else self.color.data_ptr(),
                                                 None if bricks is None else bricks.data_ptr(), views.data_ptr(), K, depth.data_ptr(),
                                                 status.data_ptr(), None if normal is None else normal.data_ptr(),
                                                 None if col is None else col.data_ptr(), stream), lib)
        return VolumeView(depth, status, normal, col, t32)

    def brick_classes(self, min_weight=1.0, library=None):
        """uint8 [bx, by, bz]: the class of every brick of 8 x 8 x 8 cells (0 mixed, 1 empty, 2 free) as ``raycast`` builds them."""
        lib = _lib.load(library)
        nb = ctypes.c_size_t()
        _lib.check(lib.vmapstep_tsdf_bricks_bytes(*self.shape, ctypes.byref(nb)), lib)
        with torch.cuda.device(self.device):
            bricks = torch.empty(nb.value, dtype=torch.uint8, device=self.device)
            _lib.check(lib.vmapstep_tsdf_bricks(*self.shape, float(min_weight), self.tsdf.data_ptr(), self.weight.data_ptr(), bricks.data_ptr(),
                                                _devmem.stream(self.device)), lib)
        bd = tuple((s + 6) >> 3 for s in self.shape)
        return bricks[:bd[0] * bd[1] * bd[2]].reshape(bd)

    def extract_mesh(self, min_weight=1.0, min_component_area=None, largest_components=None):
        """The surface as a ``Mesh`` in world coordinates, or ``None``: marching cubes at TSDF = 0 over the voxels whose weight is at
        least ``min_weight``.  The kernels call a corner 'above' where the value is greater than the level and point normals to
        decreasing values; ``Trainer.meshing`` feeds them an occupancy, high inside.  Here the negated TSDF is fed (one elementwise
        pass), high inside as well: faces are wound and normals point as ``Trainer.meshing``'s do, to free space.  With a colour volume
        every vertex gets the lerp of its edge's two voxel colours at the vertex's own parameter, rounded half to even.
        ``min_component_area`` / ``largest_components`` go through ``components.keep_components``."""
        with torch.cuda.device(self.device):
            vol = torch.neg(self.tsdf)
            mesh, edges = extract_mesh(vol, 0.0, self.affine, valid=self.weight >= float(min_weight), return_edges=True)
            if mesh is None:
                return None
            if self.color is not None:
                e = edges.long()
                p0, ax = torch.div(e, 3, rounding_mode="floor"), e % 3
                stride = torch.tensor([self.shape[1] * self.shape[2], self.shape[2], 1], device=self.device)[ax]
                flat = vol.reshape(-1)
                v0, v1 = flat[p0], flat[p0 + stride]
                t = ((0.0 - v0) / (v1 - v0)).unsqueeze(1)
                c0, c1 = self.color[p0, :3], self.color[p0 + stride, :3]
                mesh.vertex_colors = torch.round(c0 + (c1 - c0) * t).clamp_(0, 255).to(torch.uint8)
            if min_component_area is not None or largest_components is not None:
                from . import components
                mesh = components.keep_components(mesh, min_area=float(min_component_area or 0.0), largest=largest_components)
            return mesh


def fuse_object(object_keyframes, intrinsics, voxel_size, trunc, *, color=False, min_weight=1.0, min_component_area=None,
                largest_components=None, **kw):
    """The paper's per-object TSDF baseline in one call: the box from ``ObjectKeyframes.get_bound``, the object's own keyframes and its
    instance id -> the ``Mesh``, or ``None`` (no box, or no surface).  ``kw`` goes to ``integrate`` (margin, min_depth, max_depth)."""
    ok = object_keyframes
    bound = ok.get_bound(intrinsics)
    if bound is None:
        return None
    with torch.cuda.device(ok.store.device):
        vol = TSDFVolume.from_bound(bound, voxel_size=voxel_size, trunc=trunc, color=color, device=ok.store.device)
        vol.integrate_store(ok.store, intrinsics, slots=[s for s in ok.slots[:ok.n_keyframes] if s >= 0], obj_id=ok.obj_id, **kw)
        return vol.extract_mesh(min_weight, min_component_area, largest_components)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m vmap_amd.tsdf", description="fuse posed depth frames into a mesh")
    ap.add_argument("frames", metavar="FRAMES.npz", help="depth [K,W,H], t_wc [K,4,4], intrinsics [4]; optional rgb [K,W,H,3] uint8, inst [K,W,H]")
    ap.add_argument("out", metavar="OUT.ply", help=".ply or .obj")
    ap.add_argument("--voxel-size", type=float, required=True, metavar="X")
    ap.add_argument("--trunc", type=float, required=True, metavar="Y")
    ap.add_argument("--obj-id", type=int, default=None, metavar="N", help="fuse only the pixels of this instance (the file needs inst)")
    ap.add_argument("--max-depth", type=float, default=FLT_MAX)
    ap.add_argument("--min-weight", type=float, default=1.0)
    ap.add_argument("--min-component-area", type=float, default=None, metavar="X")
    ap.add_argument("--largest-components", type=int, default=None, metavar="K")
    ap.add_argument("--views", default=None, metavar="OUT.npz", help="also write the ray cast of the volume at the frames' own poses")
    args = ap.parse_args(argv)
    with np.load(args.frames) as fr:
        depth, t_wc, intrinsics = fr["depth"], fr["t_wc"], fr["intrinsics"]
        rgb = fr["rgb"] if "rgb" in fr.files else None
        inst = fr["inst"] if "inst" in fr.files else None
    if args.obj_id is not None and inst is None:
        ap.error("--obj-id needs an inst array in the frames file")
    dev = _device()
    d = torch.as_tensor(depth).to(device=dev, dtype=torch.float32)
    ins = None if inst is None else torch.as_tensor(inst.astype(np.int32)).to(dev)
    box = _box_of_frames(depth, t_wc, intrinsics, inst, args.obj_id, args.max_depth)
    vol = TSDFVolume.from_bound(box, voxel_size=args.voxel_size, trunc=args.trunc, color=rgb is not None, device=dev)
    vol.integrate(d, t_wc, intrinsics, rgb=rgb, inst=ins, obj_id=args.obj_id, max_depth=args.max_depth)
    if args.views is not None:
        usable = d[torch.isfinite(d) & (d > 0) & (d <= args.max_depth)]
        far = float(usable.max()) if usable.numel() else 1.0
        view = vol.raycast(t_wc, intrinsics, d.shape[1], d.shape[2], min_depth=0.0, max_depth=far + 2 * args.trunc, min_weight=args.min_weight)
        arrays = dict(depth=view.depth.cpu().numpy(), status=view.status.cpu().numpy(), normal=view.normal.cpu().numpy(), t_wc=view.t_wc)
        if view.color is not None:
            arrays["color"] = view.color.cpu().numpy()
        np.savez(args.views, **arrays)
        print(f"{args.views}: {len(view.t_wc)} views, {int((view.status == VolumeView.HIT).sum())} pixels hit")
    mesh = vol.extract_mesh(args.min_weight, args.min_component_area, args.largest_components)
    if mesh is None:
        print("no surface")
        return 1
    mesh.export(args.out)
    print(f"{args.out}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces, volume {vol.shape}")
    return 0


def _box_of_frames(depth, t_wc, intrinsics, inst, obj_id, max_depth):
    """The axis-aligned box of the frames' unprojected pixels (host side: the command line's one-off set-up, not a hot path)."""
    fx, fy, cx, cy = _intrinsics4(intrinsics)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    K, W, H = depth.shape
    w, h = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="ij")
    for k in range(K):
        T = np.asarray(t_wc[k], np.float64).reshape(4, 4)
        d = np.asarray(depth[k], np.float64)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(d) & (d > 0) & (d <= max_depth)
        if obj_id is not None:
            ok &= np.asarray(inst[k]) == obj_id
        if not ok.any() or not T[:3, :3].any():
            continue
        p = np.stack([(w[ok] - cx) / fx * d[ok], (h[ok] - cy) / fy * d[ok], d[ok]], -1) @ T[:3, :3].T + T[:3, 3]
        lo, hi = np.minimum(lo, p.min(0)), np.maximum(hi, p.max(0))
    if not np.isfinite(lo).all():
        raise _lib.VmapStepError("no usable depth in the frames")
    return BoundingBox((lo + hi) / 2, np.eye(3), hi - lo)


if __name__ == "__main__":
    raise SystemExit(main())
