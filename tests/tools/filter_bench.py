"""The instance filter at ScanNet frame size (620 x 460 after the 10-pixel crop, about 30 instances of which about 20 are known,
16-bit inputs already on the device): time per ``InstanceFilter.put`` and per stage - the launch groups of the C ABI (device events
around each call, median of --reps), torch's sort / merge, the box search and the host read (``InstanceFilter.stage_times``) - against
an eager torch path of the same contract in the same process on the same GPU: one full-frame mask per id, erosion by pooling, torch
unprojection, torch's floor / pack / unique for the keys.  The box search is the same code for both and is left out of the eager time.
The eager path does not pin its roundings (no fused chain), so its table is compared on the integer columns that do not depend on
them and its labels by the share of equal pixels.  Every measured ``put`` starts from the same state (restored outside the timing).

Bytes: as built filter_stats reads 6 bytes per pixel (inst, sem, depth) and writes 1 (flags); filter_write reads 4 (inst, depth) and
writes 4.  With --kernel-stats (the CSV of a rocprofv3 --kernel-trace --stats run of --trace-run) the per-kernel rates are set next
to the rate of a plain device-to-device copy of as many bytes.  A frame is 1.7 MB: all of this runs out of the caches; the copy is
the like-for-like yardstick, not the HBM peak.

    python tests/tools/filter_bench.py --out profiles/filter_bench.json [--kernel-stats profiles/filter_kernel_stats.csv]
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/tools/filter_bench.py --trace-run     # -> profiles/filter_kernel_stats.csv
"""
from __future__ import annotations

import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from vmap_amd import _devmem, _lib, instances  # noqa: E402

W, H, N_IDS, N_KNOWN = 620, 460, 30, 20
INTRINSICS = (577.6, 578.7, 318.9 - 10, 242.7 - 10)
DEPTH_SCALE, MAX_DEPTH, VOXEL = 1.0 / 1000.0, 8.0, 0.01
BACKGROUND = (1, 3)
DEV = "cuda:0"


def timed(fn, reps, before=None):
    """Median device time (ms) of fn over reps calls, events around each call on the current stream; ``before`` runs untimed."""
    out = []
    for k in range(reps + 1):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def scene(n_ids, seed=0):
    """A room-like frame [H, W]: wall and floor (background classes, ids 1 and 2) behind ellipses with ids 3 .. n_ids + 2 on a grid
    (so that each keeps most of its area), on a curved depth."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    inst = np.where(v > 0.75 * H, 1, 0).astype(np.uint16)
    sem = np.where(v > 0.75 * H, 3, 1).astype(np.uint16)
    for k in range(n_ids):
        gu, gv = k % 6, k // 6
        cu, cv = (gu + 0.5) * W / 6 + rng.uniform(-8, 8), (gv + 0.5) * H / 5 + rng.uniform(-8, 8)
        ru, rv = rng.uniform(30, 50), rng.uniform(28, 44)
        m = ((u - cu) / ru) ** 2 + ((v - cv) / rv) ** 2 <= 1.0
        inst[m] = k + 2
        sem[m] = 10 + k
    depth = (2500.0 + 600.0 * np.sin(u / 40.0) + 400.0 * np.cos(v / 35.0) + 80.0 * np.sin(u / 7.0) * np.cos(v / 6.0)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.03] = 0
    return depth, inst, sem


def eager_filter(depth, inst, sem, t_wc, box_table, state_keys, flt):
    """The contract in eager torch on the device, per-id masks as the reference loops -> (rows, labels, merged keys)."""
    ids_img = inst.to(torch.int64) + flt.id_shift
    cls = sem.to(torch.int64)
    d = depth.to(torch.float32) * DEPTH_SCALE
    d = torch.where(d > MAX_DEPTH, torch.zeros_like(d), d)
    valid = d > 0
    fx, fy, cx, cy = INTRINSICS
    v, u = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    cam = torch.stack([(u - cx) / fx * d, (v - cy) / fy * d, d, torch.ones_like(d)], -1)
    world = cam @ t_wc.t()[:, :3]
    r = flt.erode_radius
    labels = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    rows, new_keys = [], []
    for i in torch.unique(ids_img).tolist():
        mask = ids_img == i
        row = box_table[i]
        known = bool(row[15] != 0)
        mv = mask & valid
        eroded = -F.max_pool2d(-mask[None, None].float(), 2 * r + 1, 1, r)[0, 0] > 0.5
        inside = torch.zeros_like(mask)
        if known:
            proj = (world - row[0:3]) @ row[3:12].reshape(3, 3).t()
            inside = mv & (proj.abs() <= row[12:15]).all(-1)
        c = cls[mask]
        pixels, nv, ni, ne, c0, c1 = (int(x) for x in (mask.sum(), mv.sum(), inside.sum(), eroded.sum(), c.min(), c.max()))
        if c0 != c1:
            st = instances.MIXED
        elif c0 in BACKGROUND or i == 0:
            st = instances.BACKGROUND
        elif nv <= flt.min_points:
            st = instances.FEW_POINTS
        elif known:
            st = instances.UNSURE if ni == 0 else instances.MERGED
        else:
            st = instances.SMALL if ne < flt.min_pixels else instances.NEW
        emit = eroded & valid if st == instances.NEW else inside if st == instances.MERGED else None
        if emit is not None:
            k = torch.floor(world[emit] / VOXEL).to(torch.int64) + 32768
            new_keys.append((i << 48) | (k[:, 0] << 32) | (k[:, 1] << 16) | k[:, 2])
        if st == instances.NEW:
            labels[mask] = i
        elif st == instances.UNSURE:
            labels[mask] = -1
        elif st == instances.MERGED:
            labels[mask] = i
            labels[mv & ~inside] = -1
        rows.append([i, st, c0, pixels, nv, ni, ne, int((eroded & valid).sum())])
    keys = torch.unique(torch.cat([state_keys] + new_keys))
    return np.asarray(rows, np.int32), labels, keys


def kernel_stats(path):
    """{kernel name: average ns} of the filter kernels from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r["Name"].split("(")[0].replace("vf::", "")
            if name.startswith("filter_") or name == "voxel_points":
                out[name] = float(r["AverageNs"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of a rocprofv3 run of --trace-run")
    ap.add_argument("--trace-run", action="store_true", help="only the launches, 20 calls (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filter_bench needs the GPU: there is nothing to measure without one")
    flt = instances.InstanceFilter(W, H, INTRINSICS, DEPTH_SCALE, MAX_DEPTH, background_classes=BACKGROUND, voxel_size=VOXEL, device=DEV)
    first = tuple(torch.from_numpy(a).to(DEV) for a in scene(N_KNOWN))
    frame = tuple(torch.from_numpy(a).to(DEV) for a in scene(N_IDS))
    pose1 = np.eye(4, dtype=np.float32)
    pose2 = pose1.copy()
    pose2[:3, 3] = (0.03, -0.01, 0.02)
    res1 = flt.put(*first, pose1)
    snap = (flt.keys.clone(), flt.box_table.clone(), dict(flt.boxes))

    def restore():
        flt.keys, flt.boxes = snap[0].clone(), dict(snap[2])
        flt.box_table.copy_(snap[1])

    depth, inst, sem = frame
    cfg = flt._cfg(False, False, pose2)
    stream = _devmem.stream(flt.device)
    ptr = lambda t: t.data_ptr()
    labels = torch.empty(H, W, dtype=torch.int32, device=DEV)
    call_stats = lambda: _lib.check(flt.lib.vmapstep_filter_stats(ctypes.byref(cfg), ptr(depth), ptr(inst), ptr(sem), ptr(flt.box_table), ptr(flt._status),
                                                                  ptr(flt._rows_dev), flt._ws_ptr, flt._ws_bytes, stream), flt.lib)
    call_emit = lambda: _lib.check(flt.lib.vmapstep_filter_emit(ctypes.byref(cfg), ptr(depth), ptr(inst), ptr(flt._status), ptr(flt._keys_buf),
                                                                ptr(flt._rows_dev), flt._ws_ptr, flt._ws_bytes, stream), flt.lib)
    call_write = lambda: _lib.check(flt.lib.vmapstep_filter_write(ctypes.byref(cfg), ptr(depth), ptr(inst), ptr(flt.box_table), ptr(flt._status),
                                                                  ptr(labels), stream), flt.lib)
    if args.trace_run:
        for _ in range(20):
            call_stats(), call_emit(), call_write()
            flt.points(res1.new[0])
        torch.cuda.synchronize()
        return

    # the two implementations agree before anything is timed
    table = flt.box_table.clone()
    res = flt.put(*frame, pose2)
    rows, elabels, ekeys = eager_filter(depth, inst, sem, torch.from_numpy(pose2).to(DEV), table, snap[0], flt)
    counts_equal = bool(np.array_equal(rows[:, [0, 2, 3, 4, 6, 7]], res.rows[:, [0, 2, 3, 4, 6, 7]]))
    status_equal = bool(np.array_equal(rows[:, 1], np.where(res.rows[:, 1] == instances.NEW_NO_BOX, instances.NEW, res.rows[:, 1])))
    if not (counts_equal and status_equal):
        raise SystemExit("the kernels and the eager implementation disagree on the table: nothing timed")
    status = [int(s) for s in res.rows[:, 1]]
    npix = W * H
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "frame": [W, H], "ids_in_frame": len(res.rows),
               "status_counts": {instances.STATUS_NAMES[s]: status.count(s) for s in sorted(set(status))},
               "state_keys_before": int(snap[0].numel()), "state_keys_after": int(flt.keys.numel()),
               "inputs": "uint16 depth, uint16 labels, on the device",
               "eager_table_equal_on_integer_columns": True, "eager_labels_equal_share": float((elabels == res.labels).float().mean()),
               "eager_keys_equal_share": float(torch.isin(flt.keys, ekeys).float().mean()), "cases": []}

    def emit(rec):
        results["cases"].append(rec)
        print(json.dumps(rec), flush=True)

    stages, host = [], []
    for _ in range(args.reps):
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flt.put(*frame, pose2)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        stages.append(flt.stage_times())
    put_ms = statistics.median(host)
    emit({"case": "InstanceFilter.put, everything (host clock, device idle at both ends)", "ms": put_ms})
    for name in stages[0]:
        ms = statistics.median(s[name] for s in stages)
        emit({"case": f"put stage '{name}' (stream events)", "ms": ms, "share_of_put": ms / put_ms})
    restore()
    emit({"case": "vmapstep_filter_stats: filter_init, filter_stats, filter_decide", "ms": timed(call_stats, args.reps)})
    emit({"case": "vmapstep_filter_emit: filter_count, filter_scan, filter_emit", "ms": timed(call_emit, args.reps)})
    emit({"case": "vmapstep_filter_write", "ms": timed(call_write, args.reps)})
    big = max(flt.boxes, key=lambda i: int(flt._segment(flt.keys, i).numel()))
    emit({"case": "InstanceFilter.points of the largest registered cloud (segment lookup + vmapstep_voxel_points)", "ms": timed(lambda: flt.points(big), args.reps),
          "points": int(flt._segment(flt.keys, big).numel())})
    pose_t = torch.from_numpy(pose2).to(DEV)
    eager_ms = timed(lambda: eager_filter(depth, inst, sem, pose_t, snap[1], snap[0], flt), max(3, args.reps // 4))
    search_ms = statistics.median(s["search"] for s in stages)
    emit({"case": "eager torch, same contract without the box search (per-id masks, pooling erosion, torch unprojection, unique)",
          "ms": eager_ms, "put_without_search_ms": put_ms - search_ms, "times_put_without_search": eager_ms / (put_ms - search_ms)})
    for name, nbytes in (("filter_stats", 7 * npix), ("filter_write", 8 * npix)):
        half = nbytes // 2
        src, dst = torch.empty(half, dtype=torch.uint8, device=DEV), torch.empty(half, dtype=torch.uint8, device=DEV)
        copy_ms = timed(lambda: dst.copy_(src), args.reps)
        rec = {"case": f"device-to-device copy moving {name}'s {nbytes // npix} bytes per pixel", "ms": copy_ms, "bytes_per_s": 2 * half / (copy_ms * 1e-3)}
        if args.kernel_stats:
            ks = kernel_stats(args.kernel_stats)
            rate = nbytes / (ks[name] * 1e-9)
            rec.update(kernel_us=ks[name] / 1e3, kernel_bytes_per_s=rate, fraction_of_copy_rate=rate / rec["bytes_per_s"])
        emit(rec)
    if args.kernel_stats:
        ks = kernel_stats(args.kernel_stats)
        for name, ns in sorted(ks.items()):
            emit({"case": f"{name} (rocprofv3 kernel trace, average)", "us": ns / 1e3})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
