"""Mesh extraction, stage by stage (device events around each stage, median of --reps):
grid (vmapstep_mesh_grid_points), query (Trainer.eval_points on the grid), count (vmapstep_mesh_count: count + scan), count readback
(the device -> host copy of the two totals, the one synchronisation), emit (vmapstep_mesh_emit: vertices + normals, faces), colour
query (eval_points at the vertices), and the whole Trainer.meshing call (wall clock, synchronised).  For each stage the bytes it must
move at least and the rate that implies against the HBM figure of the MI355X (8 TB/s peak, about 6.3 TB/s achievable).

    python tests/tools/mesh_bench.py --dims 128 256 384 --out profiles/mesh_bench.json

Two volumes per size: an analytic sphere built on the device (count / emit only: it has no field) and a hidden-32 field with a
surface (random initialisation, out_alpha's bias shifted by the median logit; a rough surface with many faces: the heavy case).
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

from vmap_amd import _devmem, _lib, meshing  # noqa: E402
from vmap_amd.trainer import SimpleConfig, Trainer  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def timed(fn, reps):
    """Median device time (ms) of fn over reps calls, events recorded around each call on the current stream."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def mesh_stages(vol, reps):
    """count / readback / emit of one volume through the C ABI."""
    lib = _lib.load()
    shape = tuple(vol.shape)
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_mesh_workspace_bytes, vol.device, *shape)
    stream = _devmem.stream(vol.device)
    counts = torch.empty(2, dtype=torch.int64, device=vol.device)
    host = torch.empty(2, dtype=torch.int64).pin_memory()

    def count():
        _lib.check(lib.vmapstep_mesh_count(vol.data_ptr(), *shape, 0.5, counts.data_ptr(), ws_ptr, nbytes, stream), lib)

    t_count = timed(count, reps)
    count()
    t_read = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(counts)
        torch.cuda.synchronize()
        t_read.append((time.perf_counter() - t0) * 1e3)
    nv, nf = (int(x) for x in host)
    verts = torch.empty(nv, 3, device=vol.device)
    normals = torch.empty(nv, 3, device=vol.device)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=vol.device)

    def emit():
        _lib.check(lib.vmapstep_mesh_emit(vol.data_ptr(), *shape, 0.5, None, verts.data_ptr(), normals.data_ptr(), faces.data_ptr(),
                                          nv, nf, ws_ptr, nbytes, stream), lib)

    t_emit = timed(emit, reps)
    n = vol.numel()
    return {"vertices": nv, "faces": nf,
            "count_ms": t_count, "count_bytes": 5 * n, "readback_ms": statistics.median(t_read),
            "emit_ms": t_emit, "emit_bytes": 10 * n + 24 * nv + 12 * nf}


def rate(rec, stage):
    b, ms = rec[f"{stage}_bytes"], rec[f"{stage}_ms"]
    rec[f"{stage}_GBps"] = b / (ms * 1e-3) / 1e9
    rec[f"{stage}_fraction_of_hbm"] = b / (ms * 1e-3) / HBM_ACHIEVABLE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256, 384])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    results = {"device": torch.cuda.get_device_name(0), "hbm_achievable_Bps": HBM_ACHIEVABLE, "reps": args.reps, "runs": []}
    bound = meshing.BoundingBox(center=np.array([0.1, 0.2, -0.3]), R=np.eye(3), extent=np.array([1.2, 0.9, 1.0]))
    obj_center = torch.tensor(0.0)
    tr = Trainer(SimpleConfig(training_device="cuda:0", hidden_feature_size=32, obj_id=1))
    with torch.no_grad():
        pts = meshing.grid_points((32,) * 3, meshing.bound_affine(bound, tr.bound_extent, 32, obj_center))
        alpha, _ = tr.fc_occ_map(tr.pe(pts))
        tr.fc_occ_map.out_alpha.bias -= alpha.median() / 10.0      # the module scales the head by 10
    for D in args.dims:
        n = D ** 3
        t = torch.linspace(-1, 1, D, device="cuda")
        X, Y, Z = torch.meshgrid(t, t, t, indexing="ij")
        sphere = torch.sigmoid(20 * (0.6 - torch.sqrt(X * X + Y * Y + Z * Z)))
        del X, Y, Z
        rec = {"D": D, "volume": "sphere", **mesh_stages(sphere, args.reps)}
        rate(rec, "count")
        rate(rec, "emit")
        results["runs"].append(rec)
        print(json.dumps(rec), flush=True)
        del sphere
        A_grid = meshing.bound_affine(bound, tr.bound_extent, D, obj_center)
        rec = {"D": D, "volume": "field_h32"}
        rec["grid_ms"] = timed(lambda: meshing.grid_points((D,) * 3, A_grid), args.reps)
        rec["grid_bytes"] = 12 * n
        pts = meshing.grid_points((D,) * 3, A_grid)
        rec["query_ms"] = timed(lambda: tr._eval_points_hip(pts), max(3, args.reps // 3))
        rec["query_bytes"] = 28 * n
        occ, _ = tr._eval_points_hip(pts)
        del pts
        rec.update(mesh_stages(occ.view(D, D, D), args.reps))
        m = meshing.extract_mesh(occ.view(D, D, D), 0.5, meshing.bound_affine(bound, tr.bound_extent, D))
        rec["colour_query_ms"] = timed(lambda: tr._eval_points_hip(m.vertices), args.reps)
        rec["colour_query_bytes"] = 28 * rec["vertices"]
        for s in ("grid", "query", "count", "emit", "colour_query"):
            rate(rec, s)
        del occ, m
        tr.meshing(bound, obj_center, D)
        walls = []
        for _ in range(max(3, args.reps // 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.meshing(bound, obj_center, D)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        rec["trainer_meshing_ms"] = statistics.median(walls)
        results["runs"].append(rec)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
