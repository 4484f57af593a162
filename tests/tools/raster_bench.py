"""The mesh rasteriser at scene size: the ``Trainer.meshing`` mesh at 256^3 (cull_bench's) at 1200 x 680 from 1 and from 20 poses on a
ring looking inward, and the twelve-face room of the tests at 1200 x 680 from 20 poses whose walls fill every image.  Per shape the
median of --reps warm ``rasterize`` calls with device events around each Python call, and, through the C ABI with events around
each entry, how that time splits: the count call (setup of every (view, face) + the faces one lane draws), the draw call (one
record per large face + one wave per (view, face, tile) pair) and the resolve pass, with the counts of both paths.  Yardsticks in the
same run: a device-to-device copy of the key images' bytes (the resolve pass reads that much), and ``mark_visible`` in frustum mode
over the same vertices and poses (the setup pass does that projection three times per face).  There is no parent-commit time: the
capability is new.

    python tests/tools/raster_bench.py --out profiles/raster_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o raster -- python tests/tools/raster_bench.py --trace-run   # -> profiles/raster_kernel_stats.csv
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cull_bench  # noqa: E402
import raster_cases  # noqa: E402
from vmap_amd import _devmem, _lib, raster, visibility  # noqa: E402

W, H = 1200, 680
INTRINSICS = (600.0, 600.0, 599.5, 339.5)
MIN_DEPTH = 0.05
DEV = "cuda:0"


def timed(fn, reps):
    """Median device time (ms) of fn over reps calls after one warm call, events around each call on the current stream."""
    out = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def stages(v, f, t_wc, intr, reps):
    """The three ABI calls of one chunk, each timed on its own: dict(count_ms, draw_ms, resolve_ms, n_large, n_pairs)."""
    lib = _lib.load()
    K = len(t_wc)
    cfg = _lib.RasterCfg(*intr, MIN_DEPTH, 0.0, W, H)
    keys = torch.empty((K, W, H), dtype=torch.int64, device=DEV)
    depth, face = torch.empty((K, W, H), dtype=torch.float32, device=DEV), torch.empty((K, W, H), dtype=torch.int32, device=DEV)
    dropped, counts = torch.zeros(K, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.int64, device=DEV)
    nws, nlarge = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib.vmapstep_raster_workspace_bytes(len(f), K, 0, ctypes.byref(nws), ctypes.byref(nlarge)), lib)
    ws, ws_ptr = _devmem.aligned(nws.value, DEV)
    stream = _devmem.stream(torch.device(DEV))
    mesh_views = (ctypes.byref(cfg), v.data_ptr(), len(v), f.data_ptr(), len(f), t_wc.data_ptr(), None, K, keys.data_ptr())
    count = lambda: _lib.check(lib.vmapstep_raster_count(*mesh_views, dropped.data_ptr(), counts.data_ptr(), ws_ptr, nws.value, stream), lib)
    count()
    n_large, n_pairs = (int(x) for x in counts.cpu())
    out = {"n_large": n_large, "n_pairs": n_pairs, "dropped_per_view": float(dropped.float().mean()), "count_ms": timed(count, reps)}
    if n_large:
        _lib.check(lib.vmapstep_raster_workspace_bytes(len(f), K, n_large, ctypes.byref(nws), ctypes.byref(nlarge)), lib)
        large, large_ptr = _devmem.aligned(nlarge.value, DEV)
        # drawing the same pairs again changes nothing (a minimum): the draw call can be repeated on the keys the count call left
        out["draw_ms"] = timed(lambda: _lib.check(lib.vmapstep_raster_draw(*mesh_views, n_large, n_pairs, large_ptr, n_large, nlarge.value, ws_ptr,
                                                                            nws.value, stream), lib), reps)
    out["resolve_ms"] = timed(lambda: _lib.check(lib.vmapstep_raster_resolve(keys.data_ptr(), keys.numel(), depth.data_ptr(), face.data_ptr(), None,
                                                                             len(f), None, None, stream), lib), reps)
    other = torch.empty_like(keys)
    out["key_bytes"] = keys.numel() * 8
    out["d2d_copy_of_key_bytes_ms"] = timed(lambda: other.copy_(keys), reps)
    out["hit_share"] = float((face >= 0).float().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true", help="the kernels alone, a few calls each: for rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    mesh, source = cull_bench.scene_mesh(args.dim)
    v, f = mesh.vertices.contiguous(), mesh.faces.contiguous()
    centre = ((v.min(0).values + v.max(0).values) / 2).cpu().numpy().astype(np.float64)
    rv, rf = (torch.from_numpy(a).to(DEV) for a in raster_cases.box_room())
    room_poses = torch.from_numpy(np.concatenate([raster_cases.room_poses()] * 7)[:20].copy()).to(DEV)
    shapes = [("meshing mesh, 1 view", v, f, cull_bench.ring_poses(1, centre), INTRINSICS),
              ("meshing mesh, 20 views", v, f, cull_bench.ring_poses(20, centre), INTRINSICS),
              ("12-face room, 20 views", rv, rf, room_poses, raster_cases.room_intrinsics(W, H))]
    results = {"device": torch.cuda.get_device_name(0), "mesh": source, "grid": args.dim, "image": [W, H], "min_depth": MIN_DEPTH, "reps": args.reps,
               "runs": []}
    for name, vv, ff, t_wc, intr in shapes:
        draw = lambda: raster.rasterize((vv, ff), t_wc, intr, W, H, min_depth=MIN_DEPTH)
        if args.trace_run:
            for _ in range(3):
                draw()
            continue
        rec = {"shape": name, "faces": len(ff), "vertices": len(vv), "views": len(t_wc), "rasterize_ms": timed(draw, args.reps)}
        rec.update(stages(vv, ff, t_wc, intr, args.reps))
        rec["mark_visible_frustum_ms"] = timed(lambda: visibility.mark_visible(vv, None, t_wc, intr, None, size=(W, H)), args.reps)
        a = raster.rasterize((vv, ff), t_wc, intr, W, H, min_depth=MIN_DEPTH)
        rec["compare_depth_ms"] = timed(lambda: raster.compare_depth(a.depth, a.depth), args.reps)
        results["runs"].append(rec)
        print(json.dumps(rec), flush=True)
        del a
        torch.cuda.empty_cache()
    if args.out and not args.trace_run:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
