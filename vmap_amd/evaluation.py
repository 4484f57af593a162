"""Mesh evaluation on the device: the reference's metric/eval_3D_obj.py:8-41 (calc_3d_metric) and metric/metrics.py (accuracy,
completion, completion_ratio, chamfer) without trimesh or scipy.

The work is three kernel families of csrc/eval_kernels.h: cropping to an oriented box (vmapstep_clip_box_count / _emit, instead of
trimesh's slice_plane), area-weighted surface sampling (vmapstep_surface_sample, trimesh.sample.sample_surface's algorithm) and
exhaustive nearest neighbours (vmapstep_nn_distance, instead of scipy's cKDTree.query); means and ratios are reduced in float64.
Deviations from the reference, all deliberate:
- the random stream: Philox4x32-10 keyed on ``seed`` (u0 from 53 bits, r1 and r2 from 24 bits), not numpy's global generator, so
  samples are reproducible per (seed, stream, set) but differ from trimesh's draw for draw;
- the default box (``box=None``): the principal-axes box of the GT vertices (covariance eigenvectors, extents from the
  projections), not trimesh's minimum-volume ``oriented_bounds``; a caller after parity passes trimesh's box as a
  ``meshing.BoundingBox`` (centre = inverse transform's translation, R = its rotation, extent = the extents);
- cropping triangulates each clipped polygon as a fan from its first vertex, where trimesh's slice_plane triangulates otherwise:
  the cropped surface and its area are the same, so the sampling distribution is the same;
- sample coordinates are float32 (trimesh's are float64); the nearest-neighbour distances are float32 sqrtf of a float32 minimum.
"""
from __future__ import annotations

import ctypes
import json
import sys

import numpy as np
import torch

from . import _devmem, _lib
from .meshing import BoundingBox, Mesh, load_mesh

__all__ = ["accuracy", "completion", "completion_ratio", "chamfer", "nn_distance", "sample_surface", "crop_to_box",
           "principal_axes_box", "calc_3d_metric", "calc_3d_metrics"]


def _device():
    if not torch.cuda.is_available():
        raise _lib.VmapStepError("mesh evaluation runs on the GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _points(x, device):
    """[n,3] contiguous float32 on the device from a numpy array or a tensor."""
    t = torch.as_tensor(x) if not isinstance(x, torch.Tensor) else x
    t = t.to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
    return t


def _offsets(sizes, device):
    host = np.zeros(len(sizes) + 1, np.int64)
    host[1:] = np.cumsum(np.asarray(sizes, np.int64))
    return host, torch.from_numpy(host).to(device)


def _i64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def nn_distance(queries, refs, query_sizes=None, ref_sizes=None, return_index=False):
    """Euclidean distance from every query to its nearest ref of the same set, as a float32 device tensor (and the int32 index
    into ``refs`` of that ref, ties to the smallest index, with ``return_index``).  ``query_sizes`` / ``ref_sizes``: the sets'
    sizes (CSR order); default one set.  One vmapstep_nn_distance call for all sets."""
    lib = _lib.load()
    dev = _device()
    q, r = _points(queries, dev), _points(refs, dev)
    qs = [len(q)] if query_sizes is None else [int(x) for x in query_sizes]
    rs = [len(r)] if ref_sizes is None else [int(x) for x in ref_sizes]
    if len(qs) != len(rs):
        raise _lib.VmapStepError("nn_distance: query_sizes and ref_sizes need one entry per set")
    qo_h, qo_d = _offsets(qs, dev)
    ro_h, ro_d = _offsets(rs, dev)
    dist = torch.empty(len(q), dtype=torch.float32, device=dev)
    index = torch.empty(len(q), dtype=torch.int32, device=dev) if return_index else None
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_nn_workspace_bytes, dev, len(q), len(qs))
    _lib.check(lib.vmapstep_nn_distance(q.data_ptr(), len(q), qo_d.data_ptr(), _i64p(qo_h), r.data_ptr(), len(r), ro_d.data_ptr(),
                                        _i64p(ro_h), len(qs), dist.data_ptr(), None if index is None else index.data_ptr(), ws_ptr,
                                        nbytes, _devmem.stream(dev)), lib)
    del ws
    return (dist, index) if return_index else dist


def _mean(d):
    return float(d.double().mean())


def accuracy(gt_points, rec_points):
    """Mean distance from the reconstruction's points to the GT points (metrics.py: accuracy)."""
    return _mean(nn_distance(rec_points, gt_points))


def completion(gt_points, rec_points):
    """Mean distance from the GT points to the reconstruction's points (metrics.py: completion)."""
    return _mean(nn_distance(gt_points, rec_points))


def completion_ratio(gt_points, rec_points, dist_th=0.01):
    """Fraction of GT points whose distance to the reconstruction is strictly below ``dist_th`` (metrics.py: completion_ratio)."""
    return float((nn_distance(gt_points, rec_points) < dist_th).double().mean())


def chamfer(gt_points, rec_points):
    """(completion + accuracy) / 2 (metrics.py: chamfer), both directions in one launch."""
    dev = _device()
    g, r = _points(gt_points, dev), _points(rec_points, dev)
    d = nn_distance(torch.cat([g, r]), torch.cat([r, g]), [len(g), len(r)], [len(r), len(g)])
    return (_mean(d[:len(g)]) + _mean(d[len(g):])) / 2.0


def _mesh_arrays(mesh, device):
    v = _points(mesh.vertices, device)
    f = torch.as_tensor(mesh.faces).to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()
    return v, f


def _sample_sets(meshes, counts, seed=0, stream_id=0, set_base=0, randoms=None, return_face_index=False):
    """One vmapstep_surface_sample call: counts[s] points on meshes[s], [sum(counts), 3] float32 (and the face index into each
    mesh's own faces with ``return_face_index``).  ``randoms``: (u0 float64 [N], r float32 [N, 2]) device tensors (test mode)."""
    lib = _lib.load()
    dev = _device()
    vs, fs, vbase = [], [], 0
    for m in meshes:
        v, f = _mesh_arrays(m, dev)
        vs.append(v)
        fs.append(f + vbase)
        vbase += len(v)
    v = torch.cat(vs) if len(vs) > 1 else vs[0]
    f = torch.cat(fs) if len(fs) > 1 else fs[0]
    fo_h, fo_d = _offsets([len(x) for x in fs], dev)
    oo_h, oo_d = _offsets(counts, dev)
    n = int(oo_h[-1])
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    fidx = torch.empty(n, dtype=torch.int32, device=dev) if return_face_index else None
    rnd = None
    if randoms is not None:
        u0 = torch.as_tensor(randoms[0]).to(device=dev, dtype=torch.float64).contiguous()
        rr = torch.as_tensor(randoms[1]).to(device=dev, dtype=torch.float32).contiguous()
        if u0.numel() != n or rr.numel() != 2 * n:
            raise _lib.VmapStepError("sample randoms: u0 [N] and r [N, 2]")
        rnd = _lib.SurfaceRandoms(u0.data_ptr(), rr.data_ptr())
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_surface_sample_workspace_bytes, dev, len(f))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    _lib.check(lib.vmapstep_surface_sample(v.data_ptr(), len(v), f.data_ptr(), len(f), fo_d.data_ptr(), _i64p(fo_h), oo_d.data_ptr(),
                                           _i64p(oo_h), len(fs), seed, int(stream_id), int(set_base),
                                           None if rnd is None else ctypes.byref(rnd), pts.data_ptr(),
                                           None if fidx is None else fidx.data_ptr(), ws_ptr, nbytes, _devmem.stream(dev)), lib)
    del ws
    if return_face_index:
        return pts, fidx - torch.as_tensor(np.repeat(fo_h[:-1], counts), device=dev, dtype=torch.int32)
    return pts


def sample_surface(mesh, n, seed=0, stream_id=0, set_index=0):
    """``n`` points drawn on ``mesh`` (a ``meshing.Mesh`` or anything with ``vertices`` / ``faces``) with probability proportional
    to area, as a [n, 3] float32 device tensor: trimesh.sample.sample_surface's algorithm with a Philox stream keyed on ``seed``
    and counted on (point, ``set_index``, ``stream_id``)."""
    return _sample_sets([mesh], [int(n)], seed, stream_id, set_index)


def _box15(box):
    c = np.asarray(box.center, np.float64).reshape(3)
    R = np.asarray(box.R, np.float64).reshape(3, 3)
    e = np.asarray(box.extent, np.float64).reshape(3)
    return (ctypes.c_float * 15)(*np.concatenate([c, R.reshape(-1), e]).astype(np.float32).tolist())


def crop_to_box(mesh, box):
    """The part of ``mesh`` inside ``box`` (``meshing.BoundingBox``: centre, R with the box's axes as columns, full extent) as a
    ``Mesh`` of separate triangles (vertices [3T, 3], faces [[0,1,2], [3,4,5], ...], no normals), or ``None`` when nothing is left.
    Each face is clipped against the box's six half-spaces; faces inside the box are kept bit-unchanged."""
    lib = _lib.load()
    dev = _device()
    v, f = _mesh_arrays(mesh, dev)
    b = _box15(box)
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_clip_box_workspace_bytes, dev, len(f))
    count = torch.empty(1, dtype=torch.int64, device=dev)
    stream = _devmem.stream(dev)
    _lib.check(lib.vmapstep_clip_box_count(v.data_ptr(), len(v), f.data_ptr(), len(f), b, count.data_ptr(), ws_ptr, nbytes, stream), lib)
    t = int(count.cpu())                    # the one host synchronisation
    if t == 0:
        return None
    tri = torch.empty(t, 3, 3, dtype=torch.float32, device=dev)
    _lib.check(lib.vmapstep_clip_box_emit(v.data_ptr(), len(v), f.data_ptr(), len(f), b, tri.data_ptr(), t, ws_ptr, nbytes, stream), lib)
    del ws
    faces = torch.arange(3 * t, dtype=torch.int32, device=dev).reshape(t, 3)
    return Mesh(tri.reshape(-1, 3), faces, None)


def principal_axes_box(vertices):
    """The box used when no GT box is given: axes = eigenvectors of the vertices' covariance (a right-handed R, columns),
    extents = the range of the projections, centre = the middle of that range.  Not trimesh's minimum-volume oriented_bounds."""
    p = torch.as_tensor(vertices).detach().to("cpu", torch.float64).reshape(-1, 3).numpy()
    mu = p.mean(0)
    _, vec = np.linalg.eigh(np.cov((p - mu).T))
    R = vec[:, ::-1].copy()
    if np.linalg.det(R) < 0:
        R[:, 2] = -R[:, 2]
    proj = (p - mu) @ R
    lo, hi = proj.min(0), proj.max(0)
    return BoundingBox(center=mu + R @ ((lo + hi) / 2), R=R, extent=hi - lo)


def _enlarged(box):
    return BoundingBox(center=box.center, R=box.R, extent=np.asarray(box.extent, np.float64) / 0.9)


def calc_3d_metrics(pairs, N=200000, seed=0):
    """``calc_3d_metric`` for a list of (mesh_rec, mesh_gt, box or None) tuples, pair k drawing its samples as ``index=k``.
    Sampling is one call for all recs and one for all GTs; the nearest neighbours of both directions of every pair are ONE
    vmapstep_nn_distance launch.  Returns one entry per pair: [[acc], [comp], [ratio_1cm], [ratio_5cm]], or None where the crop
    leaves nothing - entry k equals ``calc_3d_metric(rec_k, gt_k, N, box_k, seed, index=k)``."""
    return _metrics([(rec, gt, box, k) for k, (rec, gt, box) in enumerate(pairs)], int(N), seed)


def calc_3d_metric(mesh_rec, mesh_gt, N=200000, box=None, seed=0, index=0):
    """eval_3D_obj.py:8-41 on the device: crop ``mesh_rec`` to ``box`` (default: ``principal_axes_box`` of the GT vertices)
    enlarged by 1/0.9, sample N points on each mesh, and return [[accuracy], [completion], [ratio < 1 cm], [ratio < 5 cm]], or None
    when the crop leaves nothing.  The samples are Philox streams keyed on ``seed`` and counted on (point, ``index``, 0 for the
    reconstruction / 1 for the GT)."""
    return _metrics([(mesh_rec, mesh_gt, box, int(index))], int(N), seed)[0]


def _metrics(items, N, seed):
    crops, gts, keep, where = [], [], [], []
    for i, (rec, gt, box, k) in enumerate(items):
        b = principal_axes_box(gt.vertices) if box is None else box
        c = crop_to_box(rec, _enlarged(b))
        if c is not None:
            crops.append(c)
            gts.append(gt)
            keep.append(k)
            where.append(i)
    out = [None] * len(items)
    if not keep:
        return out
    if keep == list(range(keep[0], keep[0] + len(keep))):
        # consecutive set indices: one segmented sampling call per stream (its sets are numbered keep[0] + s)
        rec_pts = _sample_sets(crops, [N] * len(keep), seed, 0, keep[0])
        gt_pts = _sample_sets(gts, [N] * len(keep), seed, 1, keep[0])
    else:
        rec_pts = torch.cat([_sample_sets([c], [N], seed, 0, k) for c, k in zip(crops, keep)])
        gt_pts = torch.cat([_sample_sets([g], [N], seed, 1, k) for g, k in zip(gts, keep)])
    n = len(keep)
    # queries: rec_0 .. rec_{n-1}, gt_0 .. gt_{n-1}; refs: gt_0 .. gt_{n-1}, rec_0 .. rec_{n-1}
    d = nn_distance(torch.cat([rec_pts, gt_pts]), torch.cat([gt_pts, rec_pts]), [N] * (2 * n), [N] * (2 * n))
    d = d.reshape(2, n, N).double()
    acc = d[0].mean(1).cpu().numpy()
    comp = d[1].mean(1).cpu().numpy()
    r1 = (d[1] < 0.01).double().mean(1).cpu().numpy()
    r5 = (d[1] < 0.05).double().mean(1).cpu().numpy()
    for j, i in enumerate(where):
        out[i] = [[float(acc[j])], [float(comp[j])], [float(r1[j])], [float(r5[j])]]
    return out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m vmap_amd.evaluation", description="accuracy / completion / completion ratio of a mesh")
    ap.add_argument("rec")
    ap.add_argument("gt")
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", metavar="FILE.npz", default=None,
                    help="depth [K,W,H], t_wc [K,4,4] and intrinsics [4]: both meshes are culled to what these frames saw first")
    ap.add_argument("--occlusion-eps", type=float, default=None, metavar="X",
                    help="with --frames: the occlusion tolerance in metres (default: the frustum test alone)")
    ap.add_argument("--min-component-area", type=float, default=None, metavar="X",
                    help="drop the components of REC (floaters) whose area is below X square metres, before any culling")
    ap.add_argument("--largest-components", type=int, default=None, metavar="K", help="keep only the K largest components of REC by area")
    ap.add_argument("--render-gt-depth", action="store_true",
                    help="with --frames: rasterise GT from the poses (the file needs t_wc, intrinsics and size = [width, height], no depth); "
                         "GT is culled to the faces that won a pixel, REC against GT's rasterised depth")
    ap.add_argument("--depth-l1", action="store_true",
                    help="with --frames: add depth_l1 (metres), depth_both_share and depth_gt_only_share of REC against GT, both rasterised "
                         "from the poses as loaded, before any culling")
    ap.add_argument("--min-raster-depth", type=float, default=0.05, metavar="X",
                    help="the rasteriser's near bound in metres: a face with a corner nearer than X is not drawn (default 0.05)")
    args = ap.parse_args(argv)
    rec, gt = load_mesh(args.rec), load_mesh(args.gt)
    if args.frames is None and args.occlusion_eps is not None:
        ap.error("--occlusion-eps needs --frames")
    if args.frames is None and (args.render_gt_depth or args.depth_l1):
        ap.error("--render-gt-depth and --depth-l1 need --frames")
    filtered, rastered = {}, {}
    if args.render_gt_depth or args.depth_l1:
        from . import raster
        with np.load(args.frames) as fr:
            r_twc, r_intr = fr["t_wc"], fr["intrinsics"]
            r_w, r_h = (int(x) for x in (fr["size"] if "size" in fr.files else fr["depth"].shape[1:]))
        view = dict(min_depth=args.min_raster_depth)
        if args.depth_l1:
            d = raster.depth_l1(rec, gt, r_twc, r_intr, r_w, r_h, **view)
            pixels = float(len(d["n_both"]) * r_w * r_h)
            rastered = {"depth_l1": d["depth_l1"], "depth_both_share": int(d["n_both"].sum()) / pixels,
                        "depth_gt_only_share": int(d["n_b_only"].sum()) / pixels}
    if args.min_component_area is not None or args.largest_components is not None:
        # REC only, and before visibility culling: culling cuts components apart
        from . import components
        rec, stats = components.keep_components(rec, min_area=args.min_component_area or 0.0, largest=args.largest_components, return_stats=True)
        filtered = {"min_component_area": args.min_component_area, "largest_components": args.largest_components,
                    "rec_components": len(stats), "rec_components_kept": int((stats.kept & (stats.faces > 0)).sum())}      # what the filtered mesh has
    if args.render_gt_depth:
        from . import visibility
        gt_depth = raster.rasterize(gt, r_twc, r_intr, r_w, r_h, **view).depth
        rec = None if rec is None else visibility.cull_to_views(rec, gt_depth, r_twc, r_intr, args.occlusion_eps)
        gt = raster.cull_to_raster(gt, r_twc, r_intr, r_w, r_h, **view)
    elif args.frames is not None:
        from . import visibility
        with np.load(args.frames) as fr:
            depth, t_wc, intrinsics = fr["depth"], fr["t_wc"], fr["intrinsics"]
        rec, gt = (None if m is None else visibility.cull_to_views(m, depth, t_wc, intrinsics, args.occlusion_eps) for m in (rec, gt))
    m = None if rec is None or gt is None else calc_3d_metric(rec, gt, N=args.n, seed=args.seed)
    if m is None:
        print(json.dumps({"rec": args.rec, "gt": args.gt, "result": None, **filtered, **rastered}))
        return 1
    culled = {} if args.frames is None else {"frames": args.frames, "occlusion_eps": args.occlusion_eps, "rec_faces": len(rec.faces),
                                             "gt_faces": len(gt.faces)}
    print(json.dumps({"rec": args.rec, "gt": args.gt, "n": args.n, "seed": args.seed, "accuracy": m[0][0], "completion": m[1][0],
                      "completion_ratio_1cm": m[2][0], "completion_ratio_5cm": m[3][0], **culled, **filtered, **rastered}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
