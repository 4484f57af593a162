"""The instance tracker at ScanNet frame size (620 x 460 after the 10-pixel crop, 32 detections of which 19 merge and 10 are new,
16-bit inputs already on the device), with 1, 4 and 16 candidates per detection (--candidates: the registered instances are spread
over classes so that every class has that many; classes short of it are filled with instances registered far away): time per
``InstanceTracker.put`` and per stage - the launch groups of the C ABI (device events around each call, median of --reps), torch's
sort / merge, the box search and the host read (``InstanceTracker.stage_times``) - against an eager torch path of the same contract
in the same process on the same GPU: one full-frame mask per detection, erosion by pooling, torch unprojection, one inside test per
(detection, candidate) pair, torch's floor / pack / unique for the keys.  The box search is the same code for both and is left out of
the eager time.  The eager path does not pin its roundings, so its table is compared on the integer columns that do not depend on
them.  Every measured ``put`` starts from the same state (restored outside the timing).

Next to it: ``vmapstep_filter_stats`` - untouched by the tracker; its unit compiles to the same object as before - on the same frame,
the detection rows as instance ids, each matched row's box in the filter's table, so that it does what the tracker does at one
candidate per detection: one inside test per valid pixel.

    python tests/tools/track_bench.py --out profiles/track_bench.json [--kernel-stats profiles/track_kernel_stats.csv]
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/tools/track_bench.py --trace-run --candidates 1   # -> profiles/track_kernel_stats.csv
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

from vmap_amd import _devmem, _lib, instances, tracking  # noqa: E402

W, H, N_DET, N_KNOWN, N_MERGE, N_NEW = 620, 460, 32, 20, 19, 10
INTRINSICS = (577.6, 578.7, 318.9 - 10, 242.7 - 10)
DEPTH_SCALE, MAX_DEPTH, VOXEL = 1.0 / 1000.0, 8.0, 0.02
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


def depth_image(seed):
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    depth = (2500.0 + 600.0 * np.sin(u / 40.0) + 400.0 * np.cos(v / 35.0) + 80.0 * np.sin(u / 7.0) * np.cos(v / 6.0)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.03] = 0
    return depth


def scene(cells, thin=(), seed=0):
    """A label image [H, W]: ellipses on the cells of an 8 x 4 grid, detection row k + 1 on cells[k]; the cells in ``thin`` hold a
    strip that does not survive the erosion."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    det = np.zeros((H, W), np.uint16)
    for k, cell in enumerate(cells):
        cu, cv = (cell % 8 + 0.5) * W / 8, (cell // 8 + 0.5) * H / 4
        ru, rv = (rng.uniform(30, 35), rng.uniform(44, 52)) if cell not in thin else (34.0, 5.0)
        det[((u - cu) / ru) ** 2 + ((v - cv) / rv) ** 2 <= 1.0] = k + 1
    return det


def build(cand):
    """A tracker with N_KNOWN instances in view, every class filled up to ``cand`` instances, and the measured frame:
    -> (tracker, (depth, det), det_classes, pose)"""
    trk = tracking.InstanceTracker(W, H, INTRINSICS, DEPTH_SCALE, MAX_DEPTH, background_classes=BACKGROUND, voxel_size=VOXEL, device=DEV)
    n_classes = -(-N_KNOWN // cand)
    known_class = [100 + k // cand for k in range(N_KNOWN)]
    res = trk.put(torch.from_numpy(depth_image(1)).to(DEV), torch.from_numpy(scene(range(N_KNOWN))).to(DEV), [0] + known_class, np.eye(4, dtype=np.float32))
    assert len(res.new) == N_KNOWN, res.status
    pad = n_classes * cand - N_KNOWN                          # the last class is short of `cand` instances: registered 50 m away
    if pad:
        far = np.eye(4, dtype=np.float32)
        far[0, 3] = 50.0
        res = trk.put(torch.from_numpy(depth_image(2)).to(DEV), torch.from_numpy(scene(range(pad))).to(DEV), [0] + [100 + n_classes - 1] * pad, far)
        assert len(res.new) == pad, res.status
    # the frame: cells 0 .. 18 as known, cells 20 .. 29 new, cell 30 of a background class, cell 31 too thin
    cells = list(range(N_MERGE)) + list(range(N_KNOWN, N_KNOWN + N_NEW)) + [30, 31]
    classes = [0] + known_class[:N_MERGE] + [100 + k % n_classes for k in range(N_NEW)] + [BACKGROUND[1], 100]
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.03, -0.01, 0.02)
    frame = (torch.from_numpy(depth_image(1)).to(DEV), torch.from_numpy(scene(cells, thin=(31,))).to(DEV))
    return trk, frame, classes, pose


def eager_track(depth, det, classes, t_wc, box_table, state_keys, trk):
    """The contract in eager torch on the device, per-detection masks as the reference loops -> (rows, labels, merged keys)."""
    rows_img = det.to(torch.int64) + trk.det_shift
    d = depth.to(torch.float32) * DEPTH_SCALE
    d = torch.where(d > MAX_DEPTH, torch.zeros_like(d), d)
    valid = d > 0
    fx, fy, cx, cy = INTRINSICS
    v, u = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    cam = torch.stack([(u - cx) / fx * d, (v - cy) / fy * d, d, torch.ones_like(d)], -1)
    world = cam @ t_wc.t()[:, :3]
    r = trk.erode_radius
    labels = torch.zeros(H, W, dtype=torch.int32, device=DEV)
    rows, new_keys, rank = [], [], 0
    for dd in torch.unique(rows_img).tolist():
        cls = classes[dd]
        mask = rows_img == dd
        mv = mask & valid
        eroded = -F.max_pool2d(-mask[None, None].float(), 2 * r + 1, 1, r)[0, 0] > 0.5
        pixels, nv, ne, nev = (int(x) for x in (mask.sum(), mv.sum(), eroded.sum(), (eroded & valid).sum()))
        st, idv, n_in, inside = tracking.NEW, 0, 0, None
        if dd == 0 or cls in BACKGROUND:
            st = tracking.BACKGROUND
        elif ne <= trk.min_pixels:
            st = tracking.SMALL
        elif nev <= trk.min_points:
            st = tracking.FEW_POINTS
        else:
            for i in trk._by_class.get(cls, ()):
                row = box_table[i]
                proj = (world - row[0:3]) @ row[3:12].reshape(3, 3).t()
                inside = mv & (proj.abs() <= row[12:15]).all(-1)
                n_in = int(inside.sum())
                if (n_in << 16) > trk.ratio_q * nv:
                    st, idv = tracking.MERGED, i
                    break
            if st == tracking.NEW:
                idv, rank, n_in = trk.next_id + rank, rank + 1, 0
        emit = eroded & valid if st == tracking.NEW else inside if st == tracking.MERGED else None
        if emit is not None:
            k = torch.floor(world[emit] / VOXEL).to(torch.int64) + 32768
            new_keys.append((idv << 48) | (k[:, 0] << 32) | (k[:, 1] << 16) | k[:, 2])
            labels[mask] = idv
            if st == tracking.MERGED:
                labels[mv & ~inside] = -1
        rows.append([dd, st, cls, idv, pixels, nv, n_in, ne, nev])
    keys = torch.unique(torch.cat([state_keys] + new_keys))
    return np.asarray(rows, np.int32), labels, keys


def kernel_stats(path):
    """{kernel name: average ns} of the track kernels (and filter_stats, voxel_points) from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r["Name"].split("(")[0].replace("vt::", "").replace("vf::", "")
            if name.startswith("track_") or name in ("filter_stats", "voxel_points"):
                out[name] = float(r["AverageNs"])
    return out


def calls(trk, frame, classes, pose):
    """The three launch groups of one frame as closures, on the tracker's own buffers (the pair table uploaded once)."""
    depth, det = frame
    pair_off, pair_inst = trk.pair_table(classes)
    meta = np.zeros(2 * trk.max_det + 1 + trk.max_pairs, np.int32)
    meta[:len(classes)] = classes
    meta[trk.max_det:2 * trk.max_det + 1] = pair_off
    meta[2 * trk.max_det + 1:2 * trk.max_det + 1 + pair_inst.size] = pair_inst
    trk._meta_dev.copy_(torch.from_numpy(meta))
    cfg = trk._cfg(False, False, pose, len(classes), int(pair_inst.size))
    stream = _devmem.stream(trk.device)
    ptr = lambda t: t.data_ptr()
    labels = torch.empty(H, W, dtype=torch.int32, device=DEV)
    stats = lambda: _lib.check(trk.lib.vmapstep_track_stats(ctypes.byref(cfg), ptr(depth), ptr(det), ptr(trk._meta_dev), ptr(trk.box_table), ptr(trk._status),
                                                            ptr(trk._ident), ptr(trk._rows_dev), trk._ws_ptr, trk._ws_bytes, stream), trk.lib)
    emit = lambda: _lib.check(trk.lib.vmapstep_track_emit(ctypes.byref(cfg), ptr(depth), ptr(det), ptr(trk.box_table), ptr(trk._status), ptr(trk._ident),
                                                          ptr(trk._keys_buf), ptr(trk._rows_dev), trk._ws_ptr, trk._ws_bytes, stream), trk.lib)
    write = lambda: _lib.check(trk.lib.vmapstep_track_write(ctypes.byref(cfg), ptr(depth), ptr(det), ptr(trk.box_table), ptr(trk._status), ptr(trk._ident),
                                                            ptr(labels), stream), trk.lib)
    return stats, emit, write, int(pair_inst.size)


def filter_stats_call(trk, frame, classes, res, pose):
    """vmapstep_filter_stats on the same frame: the rows as instance ids, the matched instance's box as each merged row's box."""
    depth, det = frame
    flt = instances.InstanceFilter(W, H, INTRINSICS, DEPTH_SCALE, MAX_DEPTH, background_classes=BACKGROUND, voxel_size=VOXEL, id_shift=0, max_ids=64, device=DEV)
    sem = torch.tensor(classes, dtype=torch.int64, device=DEV)[det.to(torch.int64)].to(torch.uint16)
    for d, i in res.ids.items():
        if res.status[d] == tracking.MERGED:
            flt.box_table[d] = trk.box_table[i]
    cfg = flt._cfg(False, False, pose)
    ptr = lambda t: t.data_ptr()
    keep = (flt, sem)
    return lambda: (keep, _lib.check(flt.lib.vmapstep_filter_stats(ctypes.byref(cfg), ptr(depth), ptr(det), ptr(sem), ptr(flt.box_table), ptr(flt._status),
                                                                   ptr(flt._rows_dev), flt._ws_ptr, flt._ws_bytes, _devmem.stream(flt.device)), flt.lib))


def run(cand, args, results):
    trk, frame, classes, pose = build(cand)
    snap = (trk.keys.clone(), trk.box_table.clone(), dict(trk.boxes), dict(trk.class_of), {c: list(v) for c, v in trk._by_class.items()}, trk.next_id)

    def restore():
        trk.keys, trk.boxes, trk.class_of, trk.next_id = snap[0].clone(), dict(snap[2]), dict(snap[3]), snap[5]
        trk._by_class = {c: list(v) for c, v in snap[4].items()}
        trk.box_table.copy_(snap[1])

    stats, emit_keys, write, n_pairs = calls(trk, frame, classes, pose)
    if args.trace_run:
        flt_stats = None
        for k in range(20):
            stats(), emit_keys(), write()
            if k == 0:
                res = trk.put(*frame, classes, pose)
                restore()
                flt_stats = filter_stats_call(trk, frame, classes, res, pose)
            flt_stats()
        torch.cuda.synchronize()
        return

    # the two implementations agree before anything is timed
    res = trk.put(*frame, classes, pose)
    restore()
    rows, elabels, ekeys = eager_track(*frame, classes, torch.from_numpy(pose).to(DEV), snap[1], snap[0], trk)
    cols = [0, 2, 4, 5, 7, 8]
    if not np.array_equal(rows[:, cols], res.rows[:, cols]) or not np.array_equal(rows[:, 1], np.where(res.rows[:, 1] == tracking.NEW_NO_BOX, tracking.NEW, res.rows[:, 1])):
        raise SystemExit("the kernels and the eager implementation disagree on the table: nothing timed")
    status = [int(s) for s in res.rows[:, 1]]
    per_det = np.diff(trk.pair_table(classes)[0])[1:len(classes)]
    info = {"candidates_per_detection": cand, "registered_instances": len(snap[2]), "pairs": n_pairs,
            "candidates_of_the_rows_that_have_any": sorted(set(int(x) for x in per_det if x)),
            "status_counts": {tracking.STATUS_NAMES[s]: status.count(s) for s in sorted(set(status))},
            "eager_labels_equal_share": float((elabels == res.labels).float().mean())}
    cases = []

    def emit(rec):
        rec = dict(rec, candidates=cand)
        cases.append(rec)
        print(json.dumps(rec), flush=True)

    stages, host = [], []
    for _ in range(args.reps):
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trk.put(*frame, classes, pose)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        stages.append(trk.stage_times())
    put_ms = statistics.median(host)
    emit({"case": "InstanceTracker.put, everything (host clock, device idle at both ends)", "ms": put_ms})
    for name in stages[0]:
        ms = statistics.median(s[name] for s in stages)
        emit({"case": f"put stage '{name}' (stream events)", "ms": ms, "share_of_put": ms / put_ms})
    restore()
    stats_ms = timed(stats, args.reps)
    emit({"case": "vmapstep_track_stats: track_init, track_stats, track_decide", "ms": stats_ms})
    emit({"case": "vmapstep_track_emit: track_count, track_scan, track_emit", "ms": timed(emit_keys, args.reps)})
    emit({"case": "vmapstep_track_write", "ms": timed(write, args.reps)})
    flt_ms = timed(filter_stats_call(trk, frame, classes, res, pose), args.reps)
    emit({"case": "vmapstep_filter_stats on the same frame (filter_init, filter_stats, filter_decide; one inside test per valid pixel of a merged row)",
          "ms": flt_ms, "track_stats_over_filter_stats": stats_ms / flt_ms})
    pose_t = torch.from_numpy(pose).to(DEV)
    eager_ms = timed(lambda: eager_track(*frame, classes, pose_t, snap[1], snap[0], trk), max(3, args.reps // 4))
    search_ms = statistics.median(s["search"] for s in stages)
    emit({"case": "eager torch, same contract without the box search (per-detection masks, pooling erosion, torch unprojection, one inside test per pair, unique)",
          "ms": eager_ms, "put_without_search_ms": put_ms - search_ms, "times_put_without_search": eager_ms / (put_ms - search_ms)})
    results["runs"].append(dict(info, cases=cases))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--candidates", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--kernel-stats", nargs="+", help="kernel_stats.csv files of rocprofv3 runs of --trace-run, one per --candidates value")
    ap.add_argument("--trace-run", action="store_true", help="only the launches, 20 calls (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench needs the GPU: there is nothing to measure without one")
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "frame": [W, H], "detections": N_DET,
               "inputs": "uint16 depth, uint16 label image, on the device", "voxel_size": VOXEL, "runs": []}
    for cand in args.candidates:
        run(cand, args, results)
    if args.trace_run:
        return
    for cand, path in zip(args.candidates, args.kernel_stats or ()):
        ks = kernel_stats(path)
        rec = {"candidates": cand, "source": os.path.relpath(path, ROOT), "average_us": {k: v / 1e3 for k, v in sorted(ks.items())}}
        if "filter_stats" in ks and "track_stats" in ks:
            rec["track_stats_over_filter_stats"] = ks["track_stats"] / ks["filter_stats"]
        results.setdefault("kernel_trace", []).append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
