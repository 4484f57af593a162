"""Frame ingest at Replica frame size (1200 x 680, about 60 instances, 16-bit inputs already on the device): the four launches of
vmapstep_ingest_frame (device events around each call, median of --reps; and a window of --reps calls back to back) against two
baselines in the same process on the same GPU:

  eager torch     the same contract written with torch on the device, the way the reference's loader works: torch.unique, one
                  full-frame mask per id, any / argmax for the extents, the relabel, the transposes.  Its output is compared with the
                  kernels' before anything is timed.
  FrameStore.put  fed with already labelled, already transposed device tensors.  It does strictly less work (no statistics, no boxes,
                  no transposes, no conversion); the ratio is recorded without a threshold.

Bytes: the contract moves 9 bytes in (rgb 3, depth 2, inst 2, sem 2) and 12 out (rgbx 4, depth 4, inst 4) per pixel.  As built,
ingest_stats reads 4 bytes per pixel and ingest_write reads 7 (inst a second time) and writes 12.  With --kernel-stats (the CSV of a
rocprofv3 --kernel-trace --stats run of --trace-run) the per-kernel rates are set next to the device's copy rate, measured here by a
plain device-to-device copy that moves the contract's 21 bytes per pixel (half of them read, half written).  A frame is 17 MB, so all
of these run out of the caches as much as out of HBM; the copy is the like-for-like yardstick, not the HBM peak.

    python tests/tools/ingest_bench.py --out profiles/ingest_bench.json [--kernel-stats profiles/ingest_kernel_stats.csv]
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/tools/ingest_bench.py --trace-run     # -> profiles/ingest_kernel_stats.csv
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from vmap_amd import ingest, keyframes  # noqa: E402

W, H, N_IDS = 1200, 680, 64
DEPTH_SCALE, MAX_DEPTH, BBOX_SCALE, MIN_BOX = 1.0 / 6553.5, 8.0, 0.2, 10
DEV = "cuda:0"


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


def window(fn, reps):
    """Average device time (ms) of reps calls enqueued back to back between one pair of events."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def scene(seed=0):
    """A room-like frame [H, W]: wall and floor (background classes) behind N_IDS ellipses of their own ids, later ones over earlier
    ones, sizes from a few pixels (dropped as too small) to a tenth of the frame across; a few of them of background classes."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    inst = np.zeros((H, W), np.uint16)
    sem = np.where(v > 0.7 * H, 40, 93).astype(np.uint16)
    inst[v > 0.7 * H] = 1
    for k in range(2, N_IDS + 1):
        cu, cv = rng.uniform(0, W), rng.uniform(0, H)
        ru, rv = rng.uniform(4, 0.1 * W), rng.uniform(4, 0.12 * H)
        m = ((u - cu) / ru) ** 2 + ((v - cv) / rv) ** 2 <= 1.0
        inst[m] = k + (300 if k % 7 == 0 else 0)
        sem[m] = 97 if k % 9 == 0 else 1 + k % 80
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    return rgb, depth, inst, sem


def eager_ingest(rgb, depth, inst, sem, background):
    """The contract in eager torch on the device, per-id masks as the reference builds them -> (rows, rgb [W, H, 3], depth, inst [W, H])."""
    obj = inst.to(torch.int32).t()                                            # [W, H]
    cls = sem.to(torch.int32).t()
    image = rgb.permute(1, 0, 2).contiguous()
    d = depth.to(torch.float32).t() * DEPTH_SCALE
    d = torch.where(d > MAX_DEPTH, torch.zeros_like(d), d).contiguous()
    ids = torch.unique(obj)
    keep, rows = [], []
    masks = obj.unsqueeze(0) == ids.view(-1, 1, 1)                            # one full-frame mask per id
    counts = masks.flatten(1).sum(1)
    along_u, along_v = masks.any(2), masks.any(1)
    u0 = torch.argmax(along_u.float(), 1)
    u1 = W - torch.argmax(along_u.float().flip(1), 1)
    v0 = torch.argmax(along_v.float(), 1)
    v1 = H - torch.argmax(along_v.float().flip(1), 1)
    big = torch.iinfo(torch.int32).max
    cmin = torch.where(masks, cls.unsqueeze(0), big).flatten(1).amin(1)
    cmax = torch.where(masks, cls.unsqueeze(0), -big).flatten(1).amax(1)
    table = torch.stack([ids.long(), counts, u0, u1, v0, v1, cmin.long(), cmax.long()], 1).cpu().tolist()       # the one read-back
    half = np.float32(0.5 * BBOX_SCALE)
    for i, n, a0, a1, b0, b1, c0, c1 in table:
        mu, mv = int(half * np.float32(a1 - a0)), int(half * np.float32(b1 - b0))
        st, box = ingest.KEPT, [0, 0, 0, 0]
        if c0 != c1:
            st = ingest.MIXED
        elif c0 in background:
            st = ingest.BACKGROUND
        elif a1 - a0 <= MIN_BOX or b1 - b0 <= MIN_BOX:
            st = ingest.SMALL
        elif mu == 0 or mv == 0:
            st = ingest.ZERO_MARGIN
        else:
            box = [min(max(a0 - mu, 0), W - 1), min(max(a1 + mu, 0), W - 1), min(max(b0 - mv, 0), H - 1), min(max(b1 + mv, 0), H - 1)]
            keep.append(i)
        if i == 0:
            box = [0, W, 0, H]
        rows.append([i, st, n] + box + [c0])
    kept = torch.tensor(keep, dtype=torch.int32, device=obj.device)
    out = torch.where(torch.isin(obj, kept), obj, torch.zeros_like(obj)).contiguous()
    return np.asarray(rows, np.int32), image, d, out


def kernel_stats(path):
    """{kernel name: average ns} of the ingest kernels from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r["Name"].split("(")[0].replace("vi::", "")
            if name.startswith("ingest_"):
                out[name] = float(r["AverageNs"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of a rocprofv3 run of --trace-run")
    ap.add_argument("--trace-run", action="store_true", help="only the kernels, 20 calls (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench needs the GPU: there is nothing to measure without one")
    background = ingest.REPLICA_BACKGROUND_CLASSES
    store = keyframes.FrameStore(4, W, H, device=DEV)
    ing = ingest.FrameIngest(store, DEPTH_SCALE, MAX_DEPTH, background_classes=background, bbox_scale=BBOX_SCALE, min_box=MIN_BOX)
    rgb, depth, inst, sem = (torch.from_numpy(a).to(DEV) for a in scene())
    run = lambda: ing.enqueue(0, rgb, depth, inst, sem)
    if args.trace_run:
        for _ in range(20):
            run()
        torch.cuda.synchronize()
        return

    # the two implementations agree before anything is timed
    res = ing.put(rgb, depth, inst, sem, torch.eye(4), 0)
    rows, image, d, obj = eager_ingest(rgb, depth, inst, sem, background)
    same = (np.array_equal(rows, res.rows) and torch.equal(store.rgbx[res.slot, :, :, :3], image) and torch.equal(store.depth[res.slot], d)
            and torch.equal(store.inst[res.slot], obj))
    if not same:
        raise SystemExit("the kernels and the eager implementation disagree: nothing timed")
    store.collect()
    npix = W * H
    status = [int(s) for s in res.rows[:, 1]]
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "frame": [W, H], "ids_in_frame": len(res.rows),
               "kept": status.count(ingest.KEPT), "background": status.count(ingest.BACKGROUND), "small": status.count(ingest.SMALL),
               "inputs": "uint16 depth, uint16 labels, on the device", "outputs_equal_eager_torch": True, "cases": []}

    def emit(rec):
        results["cases"].append(rec)
        print(json.dumps(rec), flush=True)

    ms = timed(run, args.reps)
    emit({"case": "vmapstep_ingest_frame: four launches, per call", "ms": ms, "ms_back_to_back": window(run, args.reps),
          "contract_bytes": 21 * npix, "contract_bytes_per_s": 21 * npix / (ms * 1e-3)})
    t0 = time.perf_counter()
    for f in range(args.reps):
        ing.put(rgb, depth, inst, sem, torch.eye(4), f)
        store.collect()
    emit({"case": "FrameIngest.put: launches + read-back of the table (host clock)", "ms": (time.perf_counter() - t0) * 1e3 / args.reps})
    eager_ms = timed(lambda: eager_ingest(rgb, depth, inst, sem, background), max(5, args.reps // 5))
    emit({"case": "eager torch, same contract (torch.unique, per-id masks, any / argmax, relabel, transposes)", "ms": eager_ms,
          "times_the_kernels": eager_ms / ms})

    def plain_put():
        store.put(image, d, obj, torch.eye(4), 0)
        store.collect()

    put_ms = timed(plain_put, args.reps)
    emit({"case": "FrameStore.put alone (labelled, transposed device tensors: strictly less work)", "ms": put_ms, "kernels_over_put": ms / put_ms})
    half = 21 * npix // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device=DEV), torch.empty(half, dtype=torch.uint8, device=DEV)
    copy_ms = timed(lambda: dst.copy_(src), args.reps)
    copy_rate = 2 * half / (copy_ms * 1e-3)
    emit({"case": "device-to-device copy moving 21 bytes per pixel", "ms": copy_ms, "bytes_per_s": copy_rate, "kernels_over_copy": ms / copy_ms})
    if args.kernel_stats:
        ks = kernel_stats(args.kernel_stats)
        moved = {"ingest_stats": 4 * npix, "ingest_write": 19 * npix}
        total = sum(ks.values())
        for name in ("ingest_init", "ingest_stats", "ingest_decide", "ingest_write"):
            rec = {"case": f"{name} (rocprofv3 kernel trace, average)", "us": ks[name] / 1e3, "share_of_the_four": ks[name] / total}
            if name in moved:
                rate = moved[name] / (ks[name] * 1e-9)
                rec.update(bytes=moved[name], bytes_per_s=rate, fraction_of_copy_rate=rate / copy_rate,
                           us_at_copy_rate=moved[name] / copy_rate * 1e6, us_over_copy_rate=ks[name] / 1e3 - moved[name] / copy_rate * 1e6)
            emit(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
