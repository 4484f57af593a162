"""The depth tracker at frame size: the corner-and-sphere scene of the tests ray-cast at 1200 x 680 and 620 x 460, three levels, (10, 5, 4)
iterations from an offset of 2 cm and 1 degree, eps = 0 so that all 19 iterations run.  Per resolution, medians of --reps warm calls
with device events around each: ``DepthTracker.track`` (the frame's pyramid, the chain, the one read-back), the chain alone through
the C ABI (38 launches, no host wait), ``vmapstep_icp_pyramid`` (three launches), and icp_reduce at every level (``vmapstep_icp_sums``
called --batch times between two events; its 232-byte memset is in the figure).  icp_solve is not timed on its own here: the chain
less its reductions, divided by 19, bounds it from above (launch gaps included); the kernel trace has its own duration.

Yardstick 1: the eager torch path of the same contract on the same device (float32 maps, float64 normal equations by torch sums,
torch.linalg.solve, the same schedule); the poses are compared entry by entry, tolerance 1e-5 - float sums and another solver.
Yardstick 2, for the level-0 reduction: a device-to-device copy of the bytes it must read, 16 per source entry and 16 per gathered
model entry.  There is no parent-commit time: the capability is new.

    python tests/tools/icp_bench.py --out profiles/icp_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o icp -- python tests/tools/icp_bench.py --trace-run   # -> profiles/icp_kernel_stats.csv
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

import icp_cases as ic  # noqa: E402
from vmap_amd import _devmem, _lib, odometry  # noqa: E402

DEV = "cuda:0"
SIZES = [(1200, 680), (620, 460)]
ITERATIONS = (10, 5, 4)
CFG = dict(odometry.DEFAULTS, eps=0.0)


def timed(fn, reps, batch=1):
    """Median device time (ms) of one fn call: reps samples after a warm one, each of `batch` calls between two events."""
    out = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b) / batch)
    return statistics.median(out)


def torch_maps(depth, intr, levels, p):
    """The contract's pyramid and normal maps in eager torch, float32: [(D, V, N, camera)] per level."""
    D = torch.where((depth > p["min_depth"]) & (depth <= p["max_depth"]), depth, torch.zeros_like(depth))
    out = []
    for level in range(levels):
        if level:
            W, H = D.shape
            wa, ha = 2 * torch.arange((W + 1) // 2, device=DEV), 2 * torch.arange((H + 1) // 2, device=DEV)
            wb, hb = (wa + 1).clamp(max=W - 1), (ha + 1).clamp(max=H - 1)
            v = torch.stack([D[a][:, b] for a, b in ((wa, ha), (wb, ha), (wa, hb), (wb, hb))])
            ok = v > 0
            n = ok.sum(0)
            big = torch.where(ok, v, torch.full_like(v, -1e30)).amax(0)
            small = torch.where(ok, v, torch.full_like(v, 1e30)).amin(0)
            D = torch.where((n > 0) & (big - small <= p["band"]), (v * ok).sum(0) / n.clamp(min=1), torch.zeros_like(big))
        s = float(1 << level)
        off = ((1 << level) - 1) / 2
        cam = (intr[0] / s, intr[1] / s, (intr[2] - off) / s, (intr[3] - off) / s)
        W, H = D.shape
        w, h = torch.meshgrid(torch.arange(W, device=DEV, dtype=torch.float32), torch.arange(H, device=DEV, dtype=torch.float32), indexing="ij")
        V = torch.stack([(w - cam[2]) / cam[0] * D, (h - cam[3]) / cam[1] * D, D], -1)
        N = torch.zeros_like(V)
        ok = (D[1:-1, 1:-1] > 0) & (D[:-2, 1:-1] > 0) & (D[2:, 1:-1] > 0) & (D[1:-1, :-2] > 0) & (D[1:-1, 2:] > 0)
        ok &= ((D[2:, 1:-1] - D[:-2, 1:-1]).abs() <= 2 * p["band"]) & ((D[1:-1, 2:] - D[1:-1, :-2]).abs() <= 2 * p["band"])
        c = torch.linalg.cross(V[2:, 1:-1] - V[:-2, 1:-1], V[1:-1, 2:] - V[1:-1, :-2])
        length = c.norm(dim=-1, keepdim=True)
        n = c / length.clamp(min=1e-30)
        n = torch.where((n * V[1:-1, 1:-1]).sum(-1, keepdim=True) > 0, -n, n)
        N[1:-1, 1:-1] = torch.where((ok & (length[..., 0] > 0))[..., None], n, torch.zeros_like(n))
        out.append((D, V, N, cam))
    return out


def torch_track(src, mod, T0, iterations, p):
    """The chain in eager torch: float32 points, float64 normal equations summed by torch, torch.linalg.solve, the Cayley update."""
    T = torch.eye(4, dtype=torch.float64, device=DEV)
    T[:3] = torch.as_tensor(np.asarray(T0).reshape(3, 4), device=DEV)
    eye6 = torch.eye(6, dtype=torch.float64, device=DEV)
    for level in range(len(iterations) - 1, -1, -1):
        (Ds, Vs, Ns, cam), (Dm, Vm, Nm, _) = src[level], mod[level]
        W, H = Ds.shape
        has = (Ns != 0).any(-1)
        Ps, Nn = Vs[has], Ns[has]
        for _ in range(iterations[len(iterations) - 1 - level]):
            T32 = T.float()
            P = Ps @ T32[:3, :3].T + T32[:3, 3]
            Nr = Nn @ T32[:3, :3].T
            z = P[:, 2]
            wf, hf = torch.round(cam[0] * P[:, 0] / z + cam[2]), torch.round(cam[1] * P[:, 1] / z + cam[3])
            ok = (z > p["min_depth"]) & (wf >= 0) & (wf <= W - 1) & (hf >= 0) & (hf <= H - 1)
            wm, hm = torch.where(ok, wf, torch.zeros_like(wf)).long(), torch.where(ok, hf, torch.zeros_like(hf)).long()
            M, Q = Nm[wm, hm], Vm[wm, hm]
            ok &= (M != 0).any(-1) & ((z - Dm[wm, hm]).abs() <= p["dist_thresh"]) & ((Nr * M).sum(-1) >= p["cos_thresh"])
            P64, M64 = P.double(), M.double()
            r = (M64 * (P64 - Q.double())).sum(-1) * ok
            J = torch.cat([M64, torch.linalg.cross(P64, M64)], -1) * ok[:, None]
            x = torch.linalg.solve(J.T @ J + p["damping"] * eye6, -(J.T @ r))
            a = 0.5 * x[3:]
            K = torch.zeros(3, 3, dtype=torch.float64, device=DEV)
            K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -a[2], a[1], a[2], -a[0], -a[1], a[0]
            aa = a @ a
            dT = torch.eye(4, dtype=torch.float64, device=DEV)
            dT[:3, :3] = ((1 - aa) * torch.eye(3, dtype=torch.float64, device=DEV) + 2 * torch.outer(a, a) + 2 * K) / (1 + aa)
            dT[:3, 3] = x[:3]
            T = dT @ T
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true", help="the kernels alone, a few calls each: for rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device(DEV)
    stream = _devmem.stream(dev)
    results = {"device": torch.cuda.get_device_name(0), "iterations_coarse_first": list(ITERATIONS), "cfg": CFG, "reps": args.reps, "batch": args.batch,
               "offset": "2 cm, 1 degree", "runs": []}
    for W, H in SIZES:
        sc = ic.corner_scene(W, H)
        depth, model = torch.from_numpy(sc["depth"]).to(DEV), torch.from_numpy(sc["model_depth"]).to(DEV)
        trk = odometry.DepthTracker(sc["intrinsics"], W, H, ITERATIONS, **CFG)
        trk.set_model(model, sc["t_wc_model"])
        track = lambda: trk.track(depth, t_wc_init=sc["t_wc_model"])
        if args.trace_run:
            for _ in range(3):
                track()
            continue
        res = track()
        rec = {"image": [W, H], "ok": res.ok, "inlier_fraction": res.inlier_fraction, "iterations_run": int((res.log[:, 2] != odometry.SKIPPED).sum()),
               "pose_error_to_truth": float(np.abs(res.t_wc64 - sc["t_wc_true"]).max()),
               "initial_pose_error": float(np.abs(sc["t_wc_model"] - sc["t_wc_true"]).max()), "track_ms": timed(track, args.reps)}
        rec["track_depth_ms"] = timed(lambda: odometry.track_depth(depth, model, sc["t_wc_model"], sc["t_wc_model"], sc["intrinsics"],
                                                                    iterations=ITERATIONS, **CFG), args.reps)      # both pyramids, as the eager path
        # the stages through the C ABI
        cfg = trk._cfg
        src, _ = odometry._build_maps(lib, cfg, depth, dev)
        rec["pyramid_ms"] = timed(lambda: _lib.check(lib.vmapstep_icp_pyramid(ctypes.byref(cfg), depth.data_ptr(), src.data_ptr(), stream), lib), args.reps, args.batch)
        n = sum(ITERATIONS)
        out = torch.zeros(12 + n * 45, dtype=torch.float64, device=DEV)
        state, state_ptr = _devmem.aligned(_lib.ICP_STATE_BYTES, dev)
        T0 = torch.from_numpy(np.ascontiguousarray(sc["T_init"])).to(DEV)
        base = out.data_ptr()

        def chain():
            out[:12] = T0
            _lib.check(lib.vmapstep_icp_track(ctypes.byref(cfg), src.data_ptr(), trk._model.data_ptr(), base, base + 96, base + 8 * (12 + 16 * n),
                                              base + 8 * (12 + 4 * n), state_ptr, stream), lib)
        rec["chain_ms"] = timed(chain, args.reps)
        sums = torch.empty(29, dtype=torch.int64, device=DEV)
        rec["reduce_us"] = {}
        for level, (w, h) in enumerate(odometry.level_sizes(W, H, 3)):
            call = lambda: _lib.check(lib.vmapstep_icp_sums(ctypes.byref(cfg), src.data_ptr(), trk._model.data_ptr(), level, T0.data_ptr(), sums.data_ptr(), stream), lib)
            rec["reduce_us"][f"level{level}_{w}x{h}"] = 1e3 * timed(call, args.reps, args.batch)
        rec["level0_reduce_us_by_grid"] = {}
        for cap in (64, 128, 256, 512, 0):                             # 0: the shipped grid
            capped = odometry._cfg(sc["intrinsics"], W, H, 3, ITERATIONS, cap, **CFG)
            call = lambda: _lib.check(lib.vmapstep_icp_sums(ctypes.byref(capped), src.data_ptr(), trk._model.data_ptr(), 0, T0.data_ptr(), sums.data_ptr(), stream), lib)
            rec["level0_reduce_us_by_grid"][str(cap)] = 1e3 * timed(call, args.reps, args.batch)
        spent = sum(k * rec["reduce_us"][name] for k, name in zip(reversed(ITERATIONS), rec["reduce_us"]))
        rec["solve_and_gaps_us_upper_bound"] = (1e3 * rec["chain_ms"] - spent) / n
        nbytes = 32 * W * H
        a, b = torch.empty(nbytes, dtype=torch.uint8, device=DEV), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        rec["level0_bytes"] = nbytes
        rec["d2d_copy_of_level0_bytes_us"] = 1e3 * timed(lambda: b.copy_(a), args.reps, args.batch)
        rec["level0_reduce_over_copy"] = rec["reduce_us"][f"level0_{W}x{H}"] / rec["d2d_copy_of_level0_bytes_us"]
        # yardstick 1
        intr = sc["intrinsics"]

        def eager():
            return torch_track(torch_maps(depth, intr, 3, CFG), torch_maps(model, intr, 3, CFG), sc["T_init"], ITERATIONS, CFG)
        T = eager().cpu().numpy()
        rec["torch_eager_track_ms"] = timed(eager, max(3, args.reps // 3))
        rec["torch_pose_max_abs_diff"] = float(np.abs(T - res.t_sm64).max())
        rec["torch_pose_tolerance"] = 1e-5
        rec["torch_pose_within_tolerance"] = bool(rec["torch_pose_max_abs_diff"] <= 1e-5)
        results["runs"].append(rec)
        print(json.dumps(rec), flush=True)
        del a, b, src, out
        torch.cuda.empty_cache()
    if args.out and not args.trace_run:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
