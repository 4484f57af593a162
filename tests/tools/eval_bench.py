"""Mesh evaluation, stage by stage (device events around each call, median of --reps): nearest neighbours (vmapstep_nn_distance) at
10k x 10k as one set and as 100 sets in one launch and at 200k x 200k; area-weighted sampling of 200k points
(vmapstep_surface_sample) and cropping (vmapstep_clip_box_count + readback + _emit) on a ~1M-face marching-cubes mesh; the whole
calc_3d_metric at N = 200k.  Nearest-neighbour rates are pairs per second against two float32 vector bounds of the MI355X, each
divided by the 9 instructions per pair the inner loop issues (three subtractions, a multiply, two FMAs, a compare and two selects):
one wave64 instruction per 4 clocks per SIMD (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3e12 lane operations per second) and the
packed-float32 rate of 64 FLOP/clk/SIMD (78.6e12 lane operations per second).

    python tests/tools/eval_bench.py --out profiles/eval_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from vmap_amd import evaluation, meshing  # noqa: E402

LANE_OPS = 256 * 4 * 16 * 2.4e9
LANE_OPS_PACKED = 2 * LANE_OPS
OPS_PER_PAIR = 9


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


def gyroid_mesh(dim=256, period=100.0, size=5.0, shift=0.0):
    """Marching cubes of a gyroid over a dim^3 grid spanning `size` metres: about 1M faces at dim 256, period 100 voxels."""
    t = torch.arange(dim, device="cuda", dtype=torch.float32) * (2 * np.pi / period)
    X, Y, Z = torch.meshgrid(t, t + shift, t, indexing="ij")
    vol = (0.5 + 0.25 * (torch.sin(X) * torch.cos(Y) + torch.sin(Y) * torch.cos(Z) + torch.sin(Z) * torch.cos(X))).contiguous()
    h = size / (dim - 1)
    return meshing.extract_mesh(vol, 0.5, np.array([[h, 0, 0, 0], [0, h, 0, 0], [0, 0, h, 0]]))


def nn_case(name, nq, nr, sets, reps, rng):
    q = torch.from_numpy(rng.uniform(0, 5, (nq * sets, 3)).astype(np.float32)).cuda()
    r = torch.from_numpy(rng.uniform(0, 5, (nr * sets, 3)).astype(np.float32)).cuda()
    ms = timed(lambda: evaluation.nn_distance(q, r, [nq] * sets, [nr] * sets), reps)
    pairs = float(nq) * nr * sets
    rate = pairs / (ms * 1e-3)
    bound, packed = LANE_OPS / OPS_PER_PAIR, LANE_OPS_PACKED / OPS_PER_PAIR
    return {"case": name, "queries": nq, "refs": nr, "sets": sets, "ms": ms, "pairs_per_s": rate, "valu_bound_pairs_per_s": bound,
            "fraction_of_bound": rate / bound, "packed_rate_bound_pairs_per_s": packed, "fraction_of_packed_rate_bound": rate / packed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": []}

    def emit(rec):
        results["cases"].append(rec)
        print(json.dumps(rec), flush=True)

    emit(nn_case("nn 10k x 10k x 1", 10000, 10000, 1, args.reps, rng))
    emit(nn_case("nn 10k x 10k x 100 sets", 10000, 10000, 100, args.reps, rng))
    emit(nn_case("nn 200k x 200k", 200000, 200000, 1, max(3, args.reps // 3), rng))

    mesh = gyroid_mesh()
    nf = int(mesh.faces.shape[0])
    emit({"case": "sample 200k points", "faces": nf, "ms": timed(lambda: evaluation.sample_surface(mesh, 200000, seed=1), args.reps)})
    a = 0.5
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    box = meshing.BoundingBox(center=[2.4, 2.6, 2.5], R=Rz, extent=[3.0, 2.5, 3.5])
    crop = evaluation.crop_to_box(mesh, box)
    emit({"case": "clip to a box", "faces": nf, "triangles_out": int(crop.faces.shape[0]),
          "ms": timed(lambda: evaluation.crop_to_box(mesh, box), args.reps)})
    other = gyroid_mesh(shift=0.02)
    gt_box = meshing.BoundingBox(center=[2.5, 2.5, 2.5], R=np.eye(3), extent=[5, 5, 5])
    emit({"case": "calc_3d_metric N=200k", "faces_rec": nf, "faces_gt": int(other.faces.shape[0]),
          "ms": timed(lambda: evaluation.calc_3d_metric(mesh, other, N=200000, box=gt_box), max(3, args.reps // 3)),
          "metric": evaluation.calc_3d_metric(mesh, other, N=200000, box=gt_box)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
