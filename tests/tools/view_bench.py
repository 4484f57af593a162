"""View rendering at Replica frame size: 1200 x 680, 20 objects, S = 16 (device events around each call, one warm-up, median and
spread of --reps).

Reported: ms per view (render_view as the user calls it: count, the host read of the pair count, emit, pack, field, composite), pairs
and samples per view; the render call without the count (vmapstep_view_render alone: emit + pack + field_query_seg_s32 + composite)
next to Trainer.eval_points (pack + field_query_s32) on the same number of materialised points, alternated in the same run, both as
samples per second; and the eager path the renderer replaces (torch ray / box arithmetic, the points materialised, eval_points object
by object, sort and cumprod) on the same view.  Per-kernel times come from a kernel trace of --trace-run:

    python tests/tools/view_bench.py --out profiles/view_bench.json
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/tools/view_bench.py --trace-run       # -> profiles/view_kernel_stats.csv
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from vmap_amd import render, synth  # noqa: E402
from vmap_amd.meshing import BoundingBox  # noqa: E402
from vmap_amd.trainer import SimpleConfig, Trainer  # noqa: E402

W, H, FX, N_OBJ, S, MIN_DEPTH = 1200, 680, 600.0, 20, 16, 0.05
K4 = (FX, FX, (W - 1) / 2.0, (H - 1) / 2.0)
DEV = "cuda:0"


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "reps": reps}


def scene(seed=0):
    """20 oriented boxes on a 5 x 4 grid in the plane z = 0, seen from a ring pose at radius 3.5; random-init fields."""
    rng = np.random.default_rng(seed)
    boxes = []
    for k in range(N_OBJ):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        c = np.array([(k % 5 - 2) * 0.8, (k // 5 - 1.5) * 0.8, 0.0]) + rng.uniform(-0.1, 0.1, 3)
        boxes.append(BoundingBox(center=c.astype(np.float32), R=R.astype(np.float32), extent=rng.uniform(0.4, 0.8, 3).astype(np.float32)))
    az, el, radius = 0.4, 0.6, 3.5
    pos = radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    zc = -pos / np.linalg.norm(pos)
    xc = np.cross(zc, [0.0, 0.0, 1.0])
    xc /= np.linalg.norm(xc)
    T = np.eye(4, dtype=np.float32)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = xc, np.cross(zc, xc), zc, pos
    fc, B, sc = synth.make_params(N_OBJ, 32, seed=5)
    fields = ([torch.from_numpy(a).to(DEV) for a in fc], torch.from_numpy(B).to(DEV), torch.from_numpy(sc).to(DEV))
    centers = np.stack([np.asarray(b.center) for b in boxes]).astype(np.float32)
    return fields, boxes, T, centers


def eager_view(fields, trainers, boxes, T, centers):
    """The op stream the renderer replaces: torch rays and slabs, [pixels x objects x samples x 3] points, eval_points per object, sort,
    cumprod.  Same contract up to the rounding of the torch operations."""
    fc, B, sc = fields
    Tt = torch.from_numpy(T).to(DEV)
    w, h = torch.meshgrid(torch.arange(W, device=DEV, dtype=torch.float32), torch.arange(H, device=DEV, dtype=torch.float32), indexing="ij")
    dc = torch.stack([(w - K4[2]) / K4[0], (h - K4[3]) / K4[1], torch.ones_like(w)], -1).reshape(-1, 3)
    d = dc @ Tt[:3, :3].T
    o = Tt[:3, 3]
    P = W * H
    ts = torch.full((P, N_OBJ, S), float("inf"), device=DEV)
    occ = torch.zeros(P, N_OBJ, S, device=DEV)
    rgb = torch.zeros(P, N_OBJ, S, 3, device=DEV)
    steps = torch.arange(S, device=DEV, dtype=torch.float32) + 0.5
    for k, b in enumerate(boxes):
        R = torch.as_tensor(np.asarray(b.R), device=DEV, dtype=torch.float32)
        c = torch.as_tensor(np.asarray(b.center), device=DEV, dtype=torch.float32)
        e = torch.as_tensor(np.asarray(b.extent), device=DEV, dtype=torch.float32)
        ob, db = (o - c) @ R, d @ R
        ta, tb = (-0.5 * e - ob) / db, (0.5 * e - ob) / db
        near = torch.minimum(ta, tb).amax(1).clamp_min(MIN_DEPTH)
        far = torch.maximum(ta, tb).amin(1)
        idx = torch.nonzero(far > near).reshape(-1)
        if idx.numel() == 0:
            continue
        t = near[idx, None] + steps[None] * ((far - near)[idx, None] / S)
        pts = (o[None, None] + d[idx, None, :] * t[..., None]) - torch.from_numpy(centers[k]).to(DEV)
        oc, co = trainers[k]._eval_points_hip(pts.reshape(-1, 3))
        ts[idx, k], occ[idx, k], rgb[idx, k] = t, oc.view(-1, S), co.view(-1, S, 3)
    ts, occ, rgb = ts.reshape(P, -1), occ.reshape(P, -1), rgb.reshape(P, -1, 3)
    ts, order = ts.sort(dim=1, stable=True)
    occ = occ.gather(1, order)
    rgb = rgb.gather(1, order[..., None].expand(-1, -1, 3))
    ts = torch.where(torch.isfinite(ts), ts, torch.zeros_like(ts))
    free = torch.cat([torch.ones(P, 1, device=DEV), (1.0 - occ + 1e-10)[:, :-1]], 1)
    wgt = occ * torch.cumprod(free, 1)
    return (wgt * ts).sum(1), (wgt[..., None] * rgb).sum(1), wgt.sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true", help="three views and three point queries only: the run to put under a kernel trace")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    fields, boxes, T, centers = scene()
    kw = dict(samples=S, min_depth=MIN_DEPTH, centers=centers, budget_bytes=1 << 40)
    view = render.render_view(fields, boxes, T, K4, W, H, return_samples=True, **kw)
    n_pts = view.n_pairs * S
    tr = Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=32, obj_scale=2.0))
    pts = (torch.rand(n_pts, 3, device=DEV) - 0.5)
    if a.trace_run:
        for _ in range(3):
            render.render_view(fields, boxes, T, K4, W, H, **kw)
            tr._eval_points_hip(pts)
        torch.cuda.synchronize()
        return
    res = {"tool": "view_bench", "width": W, "height": H, "objects": N_OBJ, "samples": S, "pairs_per_view": view.n_pairs, "samples_per_view": n_pts,
           "overflow_pixels": view.overflow, "device": torch.cuda.get_device_name(0)}
    res["render_view"] = timed(lambda: render.render_view(fields, boxes, T, K4, W, H, **kw), a.reps)
    # the render call alone against the point query on as many points, alternated
    import ctypes
    from vmap_amd import _devmem, _lib
    lib = _lib.load()
    fc, pe_B, scale = fields
    pp = _lib.Params()
    for t, p in enumerate(fc):
        pp.fc[t] = _lib.Tensor(p.data_ptr(), p.stride(0))
    pp.pe_B = _lib.Tensor(pe_B.data_ptr(), pe_B.stride(0))
    sc = _lib.Tensor(scale.data_ptr(), 1)
    cfg = _lib.ViewCfg(W, H, S, N_OBJ, *K4, (ctypes.c_float * 16)(*T.reshape(-1)), MIN_DEPTH, 0, W * H)
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_view_workspace_bytes, DEV, ctypes.byref(cfg))
    boxes_d = torch.from_numpy(render._box_rows(boxes, N_OBJ)).to(DEV)
    centers_d = torch.from_numpy(centers).to(DEV)
    off_d = torch.empty(N_OBJ + 1, dtype=torch.int64, device=DEV)
    _lib.check(lib.vmapstep_view_count(ctypes.byref(cfg), boxes_d.data_ptr(), off_d.data_ptr(), ws_ptr, nbytes, _devmem.stream(DEV)), lib)
    off_h = off_d.cpu().numpy().copy()
    m = int(off_h[-1])
    bufs = [torch.empty(m, 4, dtype=torch.int32, device=DEV), torch.empty(m, S, device=DEV), torch.empty(m, S, 3, device=DEV), torch.empty(W, H, device=DEV),
            torch.empty(W, H, 3, device=DEV), torch.empty(W, H, device=DEV), torch.empty(W, H, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)]

    def call_render():
        _lib.check(lib.vmapstep_view_render(ctypes.byref(cfg), 32, ctypes.byref(pp), ctypes.byref(sc), boxes_d.data_ptr(), centers_d.data_ptr(),
                                            off_d.data_ptr(), off_h.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), bufs[0].data_ptr(), m,
                                            *(b.data_ptr() for b in bufs[1:]), ws_ptr, nbytes, _devmem.stream(DEV)), lib)

    rounds = {"view_render_call": [], "eval_points_call": []}
    for _ in range(3):                                             # alternated: each leg sees the same machine state
        rounds["view_render_call"].append(timed(call_render, a.reps))
        rounds["eval_points_call"].append(timed(lambda: tr._eval_points_hip(pts), a.reps))
    for k, v in rounds.items():
        med = [r["median_ms"] for r in v]
        res[k] = {"median_ms_per_round": med, "samples_per_s": n_pts / (statistics.median(med) * 1e-3),
                  "spread_over_rounds": (max(med) - min(med)) / statistics.median(med)}
    if not a.no_eager:
        trainers = []
        for k in range(N_OBJ):
            t = Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=32, obj_scale=2.0))
            with torch.no_grad():
                for p, src in zip(list(t.fc_occ_map.parameters()) + [t.pe.B_layer.weight], list(fc) + [pe_B]):
                    p.copy_(src[k])
            trainers.append(t)
        res["eager_torch"] = timed(lambda: eager_view(fields, trainers, boxes, T, centers), max(2, a.reps // 3))
        ed, _, eo = eager_view(fields, trainers, boxes, T, centers)
        res["eager_vs_kernel_max_abs"] = {"depth": float((ed.view(W, H) - view.depth).abs().max()), "opacity": float((eo.view(W, H) - view.opacity).abs().max())}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
