"""Object bounds, stage by stage (device events around each call, median of --reps): the unprojection (vmapstep_unproject_count +
readback + _emit) of 20 keyframes at Replica frame size (1200 x 680) for 1 and for 20 objects, one coarse vmapstep_obb_extents
launch (16384 shared candidates) over those clouds, the whole get_bounds for 1 and 20 objects, and the numpy backend's time for the
same search on the host (one object, thinned to --host-points points) for comparison.

The extents rate is (point, candidate) pairs per second against the float32 vector bound of the MI355X divided by the 15
instructions per pair the inner loop issues (a multiply, two FMAs and a min / max pair per axis): one wave64 instruction per 4
clocks per SIMD = 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3e12 lane operations per second, and against twice that, the packed
float32 rate of 64 FLOP/clk/SIMD.  (The compiled loop issues fewer than 15: it folds the minima / maxima of two consecutive points
into v_min3_f32 / v_max3_f32, about 12 instructions per pair; the bound is kept at the source's count.)

The scene is synthetic: every object is a disc of its own instance id in every frame, at a depth varying with the pixel, the 20
discs together covering about a fifth of the frame (the single-object case: one disc of that total area).

    python tests/tools/bounds_bench.py --out profiles/bounds_bench.json
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/tools/bounds_bench.py --trace-run      # -> profiles/bounds_kernel_stats.csv
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from vmap_amd import bounds, keyframes  # noqa: E402

LANE_OPS = 256 * 4 * 16 * 2.4e9
LANE_OPS_PACKED = 2 * LANE_OPS
OPS_PER_PAIR = 15
W, H, FRAMES = 1200, 680, 20
K4 = (600.0, 600.0, 599.5, 339.5)


def timed(fn, reps):
    """Median device time (ms) of fn over reps calls, events recorded around each call on the current stream."""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def scene(n_obj, area_fraction=0.2, seed=0):
    """FrameStore of FRAMES frames with n_obj discs (ids 1 .. n_obj) of equal area, together area_fraction of the frame, and the
    objects' keyframe tables (every frame a keyframe of every object)."""
    rng = np.random.default_rng(seed)
    store = keyframes.FrameStore(FRAMES, W, H, device="cuda:0")
    radius = np.sqrt(area_fraction * W * H / (np.pi * n_obj))
    cols = int(np.ceil(np.sqrt(n_obj * W / H)))
    rows = int(np.ceil(n_obj / cols))
    w, h = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    slots = []
    for f in range(FRAMES):
        inst = np.zeros((W, H), np.int32)
        for o in range(n_obj):
            cx, cy = (o % cols + 0.5) * W / cols, (o // cols + 0.5) * H / rows
            inst[(w - cx) ** 2 + (h - cy) ** 2 <= radius * radius] = o + 1
        depth = (2.0 + 0.5 * np.sin(w / 90.0 + f) * np.cos(h / 70.0) + 0.01 * rng.random((W, H))).astype(np.float32)
        a = 2 * np.pi * f / FRAMES
        t_wc = np.eye(4, dtype=np.float32)
        t_wc[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        t_wc[:3, 3] = (-2.5 * np.sin(a), 0.0, -2.5 * np.cos(a))
        slots.append(store.put(torch.zeros(W, H, 3, dtype=torch.uint8), torch.from_numpy(depth), torch.from_numpy(inst), torch.from_numpy(t_wc), f))
    objs = []
    for o in range(n_obj):
        ok = keyframes.ObjectKeyframes(store, o + 1, slots[0], (0, 0, W, H), keyframe_buffer_size=FRAMES)
        for s in slots[1:]:
            ok.append(s, (0, 0, W, H))
        objs.append(ok)
    return store, objs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-points", type=int, default=20000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true", help="only get_bounds for 1 and 20 objects, twice each: the run to put under a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bounds_bench measures on the GPU: no device found")
    if args.trace_run:
        for n_obj in (1, 20):
            _, objs = scene(n_obj)
            for _ in range(2):
                bounds.get_bounds(objs, K4)
        torch.cuda.synchronize()
        return
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "frame": [W, H], "keyframes": FRAMES,
               "search": {k: getattr(bounds, k) for k in ("COARSE_DIRECTIONS", "COARSE_ANGLES", "SEEDS", "ROUNDS", "GRID", "FINAL_STEP_DEG")},
               "cases": []}

    def emit(rec):
        results["cases"].append(rec)
        print(json.dumps(rec), flush=True)

    coarse = torch.from_numpy(np.array(bounds.coarse_rotations(), np.float32)).cuda()
    for n_obj in (1, 20):
        store, objs = scene(n_obj)
        pts, off = bounds.object_points(objs, K4)
        n = int(off[-1])
        emit({"case": f"unproject, {n_obj} object(s)", "pairs": n_obj * FRAMES, "pixels_scanned": n_obj * FRAMES * W * H, "points": n,
              "ms": timed(lambda: bounds.object_points(objs, K4), args.reps)})
        centre = torch.stack([pts[off[o]:off[o + 1]].mean(0) for o in range(n_obj)])
        ms = timed(lambda: bounds.extents(pts, coarse, off, center=centre), args.reps)
        pairs = float(n) * len(coarse)
        emit({"case": f"obb_extents coarse launch, {n_obj} object(s)", "points": n, "candidates": len(coarse), "ms": ms,
              "pairs_per_s": pairs / (ms * 1e-3), "valu_bound_pairs_per_s": LANE_OPS / OPS_PER_PAIR,
              "fraction_of_bound": pairs / (ms * 1e-3) / (LANE_OPS / OPS_PER_PAIR),
              "packed_rate_bound_pairs_per_s": LANE_OPS_PACKED / OPS_PER_PAIR,
              "fraction_of_packed_rate_bound": pairs / (ms * 1e-3) / (LANE_OPS_PACKED / OPS_PER_PAIR)})
        emit({"case": f"oriented_bounds (search only), {n_obj} object(s)", "points": n,
              "ms": timed(lambda: bounds.oriented_bounds(pts, off), max(3, args.reps // 3))})
        boxes = bounds.get_bounds(objs, K4)
        emit({"case": f"get_bounds, {n_obj} object(s)", "points": n, "ms": timed(lambda: bounds.get_bounds(objs, K4), max(3, args.reps // 3)),
              "extent_of_object_0": [float(v) for v in boxes[0].extent]})
        if n_obj == 1:
            host = pts[:: max(1, n // args.host_points)].cpu().numpy()
            t0 = time.perf_counter()
            bounds.oriented_bounds(host, backend="numpy")
            emit({"case": "oriented_bounds, numpy backend on the host, 1 object (thinned)", "points": len(host),
                  "ms": (time.perf_counter() - t0) * 1e3})
        del store, objs, pts
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
