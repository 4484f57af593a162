"""The TSDF ray cast at scene size: tsdf_bench.py's scene - a 256^3 volume (1 cm voxels) fused from 20 frames of 1200 x 680 - read out
as 1200 x 680 depth, status and normal images from 1 and from 20 of the frames' poses.  Device events around each call, median of --reps
after a warm call.

What is timed:
- ``TSDFVolume.raycast`` as the public call (the brick classes rebuilt inside, the views uploaded, the images allocated) for 1 and 20
  views, with ``use_bricks`` True and False - the condition under which the classes stay in the product path is that True is not slower;
- the ``vmapstep_tsdf_raycast`` entry alone on preallocated images, with a prebuilt class table and with none;
- ``vmapstep_tsdf_bricks`` alone, against device-to-device copies: of the 128 MB it reads (a copy reads and writes them), and of half
  of that (a copy that moves 128 MB in total).  A copy of less than 256 MB is partly served by the Infinity Cache: the yardstick
  flatters the copy, never the kernel;
- the only route to the same image without the ray cast, in the same run: ``extract_mesh()`` followed by ``raster.rasterize`` for one
  pose - the denominator of any speed-up quoted;
- the agreement of the two routes (``raster.compare_depth``), as a sanity check of the scene, not as a test.

    python tests/tools/raycast_bench.py --out profiles/raycast_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o raycast -- python tests/tools/raycast_bench.py --trace-run   # -> profiles/raycast_kernel_stats.csv
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import tsdf_bench as tb  # noqa: E402
from vmap_amd import _devmem, _lib, raster  # noqa: E402

W, H, K, DEV = tb.W, tb.H, tb.K, tb.DEV
MIN_DEPTH = 0.1


def fused_volume(data):
    depth, inst, rgbx, t_wc = data
    vol, voxel = tb.volume("scene", False)
    vol.integrate(depth, t_wc, tb.INTRINSICS, max_depth=tb.MAX_DEPTH)
    return vol, voxel


def entry_alone(vol, poses, bricks, reps):
    """vmapstep_tsdf_raycast on preallocated images; bricks: a prebuilt table or None."""
    lib = _lib.load()
    view = vol.raycast(poses, tb.INTRINSICS, W, H, min_depth=MIN_DEPTH, max_depth=tb.MAX_DEPTH)        # for the images and the cfg's inputs
    A4 = np.eye(4)
    A4[:3] = vol.affine
    M = np.stack([(np.linalg.inv(A4) @ T.astype(np.float64))[:3].reshape(12) for T in view.t_wc]).astype(np.float32)
    views = torch.from_numpy(M).to(DEV)
    nmap = (ctypes.c_float * 9)(*np.linalg.inv(vol.affine[:, :3]).T.astype(np.float32).reshape(-1).tolist())
    fx, fy, cx, cy = tb.INTRINSICS
    cfg = _lib.RaycastCfg(*vol.shape, W, H, 4096, 0, 0, fx, fy, cx, cy, MIN_DEPTH, tb.MAX_DEPTH, vol.trunc / 2, 1.0, nmap, 0.0)
    stream = _devmem.stream(torch.device(DEV))

    def call():
        _lib.check(lib.vmapstep_tsdf_raycast(ctypes.byref(cfg), vol.tsdf.data_ptr(), vol.weight.data_ptr(), None,
                                             None if bricks is None else bricks.data_ptr(), views.data_ptr(), len(M), view.depth.data_ptr(),
                                             view.status.data_ptr(), view.normal.data_ptr(), None, stream), lib)
    return tb.timed(call, reps)


def bricks_alone(vol, reps):
    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.vmapstep_tsdf_bricks_bytes(*vol.shape, ctypes.byref(nb)), lib)
    bricks = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    stream = _devmem.stream(torch.device(DEV))
    call = lambda: _lib.check(lib.vmapstep_tsdf_bricks(*vol.shape, 1.0, vol.tsdf.data_ptr(), vol.weight.data_ptr(), bricks.data_ptr(), stream), lib)
    return tb.timed(call, reps), bricks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-run", action="store_true", help="a few calls of every kernel and nothing else, for a rocprofv3 kernel trace")
    args = ap.parse_args()
    data = tb.frames()
    vol, voxel = fused_volume(data)
    poses = data[3].cpu().numpy()
    kw = dict(min_depth=MIN_DEPTH, max_depth=tb.MAX_DEPTH)
    if args.trace_run:
        for n_views in (1, K):
            for use in (True, False):
                for _ in range(3):
                    vol.raycast(poses[:n_views], tb.INTRINSICS, W, H, use_bricks=use, **kw)
        torch.cuda.synchronize()
        return
    reps = args.reps
    out = {"voxels": vol.tsdf.numel(), "voxel_size_m": voxel, "trunc_m": vol.trunc, "step_m": vol.trunc / 2, "image": [W, H]}
    classes = vol.brick_classes().cpu().numpy()
    out["bricks"] = {"total": int(classes.size), "mixed": int((classes == 0).sum()), "empty": int((classes == 1).sum()), "free": int((classes == 2).sum())}
    ms_bricks, table = bricks_alone(vol, reps)
    src = torch.empty(2 * vol.tsdf.numel() * 4, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    ms_copy_full = tb.timed(lambda: dst.copy_(src), reps)
    half = src.numel() // 2
    ms_copy_half = tb.timed(lambda: dst[:half].copy_(src[:half]), reps)
    out["tsdf_bricks"] = {"ms": ms_bricks, "bytes_read": int(src.numel()), "copy_of_the_bytes_it_reads_ms": ms_copy_full,
                          "copy_moving_as_many_bytes_in_total_ms": ms_copy_half, "bricks_over_copy_of_the_bytes_it_reads": ms_bricks / ms_copy_full,
                          "bricks_over_copy_moving_as_many_bytes": ms_bricks / ms_copy_half}
    calls = {}
    for n_views in (1, K):
        p = poses[:n_views]
        with_classes = tb.timed(lambda: vol.raycast(p, tb.INTRINSICS, W, H, use_bricks=True, **kw), reps)
        without = tb.timed(lambda: vol.raycast(p, tb.INTRINSICS, W, H, use_bricks=False, **kw), reps)
        entry_with, entry_without = entry_alone(vol, p, table, reps), entry_alone(vol, p, None, reps)
        view = vol.raycast(p, tb.INTRINSICS, W, H, **kw)
        status = np.bincount(view.status.cpu().numpy().reshape(-1), minlength=5)
        calls[str(n_views)] = {"views": n_views, "raycast_ms_with_classes": with_classes, "raycast_ms_without_classes": without,
                               "raycast_ms_per_view_with_classes": with_classes / n_views, "with_over_without": with_classes / without,
                               "entry_alone_ms_with_classes": entry_with, "entry_alone_ms_without_classes": entry_without,
                               "entry_alone_with_over_without": entry_with / entry_without,
                               "pixels": {"miss": int(status[0]), "hit": int(status[1]), "left": int(status[2]), "behind": int(status[3]), "steps": int(status[4])}}
    out["raycast"] = calls
    out["leap"] = "not built"
    # the route without the ray cast: the volume meshed, the mesh rasterised at one pose
    ms_mesh = tb.timed(lambda: vol.extract_mesh(), max(1, reps // 3))
    mesh = vol.extract_mesh()
    ms_raster = tb.timed(lambda: raster.rasterize(mesh, poses[:1], tb.INTRINSICS, W, H, min_depth=MIN_DEPTH), max(1, reps // 3))
    both = tb.timed(lambda: raster.rasterize(vol.extract_mesh(), poses[:1], tb.INTRINSICS, W, H, min_depth=MIN_DEPTH), max(1, reps // 3))
    r = raster.rasterize(mesh, poses[:1], tb.INTRINSICS, W, H, min_depth=MIN_DEPTH)
    cmp_ = raster.compare_depth(vol.raycast(poses[:1], tb.INTRINSICS, W, H, **kw).depth, r.depth)
    out["mesh_route_one_pose"] = {"extract_mesh_ms": ms_mesh, "rasterize_ms": ms_raster, "extract_mesh_then_rasterize_ms": both, "mesh_faces": len(mesh.faces),
                                  "over_raycast_one_view": both / calls["1"]["raycast_ms_with_classes"],
                                  "agreement": {k: (float(v[0]) if k == "l1" else int(v[0])) for k, v in cmp_.items()}}
    doc = {"tool": "tests/tools/raycast_bench.py", "device": torch.cuda.get_device_name(0), "frames_fused": K, "reps": reps,
           "timing": "median of device events around each call, warm", **out}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
