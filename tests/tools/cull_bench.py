"""Visibility culling at scene size: the vertices of a ``Trainer.meshing`` mesh at 256^3 against 20 and 200 frames of 1200 x 680 on a
ring of poses looking inward, with the occlusion test and with the frustum alone.  Time per ``mark_visible`` and per ``cull_mesh``
(device events around each call, median of --reps, warm) against an eager torch path of the same contract in the same process on
the same inputs: frame by frame with [n] intermediates, every fused multiply-add emulated through a float64 product so that its
flags can be - and are - required to equal the kernel's; the same path in plain float32 (what one would write first) is timed too
and its differing flags are counted.  There is no parent-commit time: the capability is new.

The depth images are a z-buffer of the mesh's own vertices (the nearest vertex per pixel), so the front of the surface passes the
occlusion test and the back does not.  A third mode, "occlusion_none_seen", replaces every measured depth by 0.5 m, in front of every
vertex: nothing is seen, no early exit helps, every pair inside a frustum gathers a depth, and the time is that of all the work.

Early exits.  How many (vertex, frame) pairs cull_mark evaluates depends on when a workgroup of a later frame chunk reads the `seen`
bytes the earlier chunks wrote, which no launch fixes.  The tool therefore reports two bounds computed from the flags of every frame:
``share_lower`` - a lane stops at the first frame that sees its vertex, chunks in order, every earlier chunk's writes visible - and
``share_upper`` - no workgroup learns anything from another chunk (a lane stops at the first seeing frame of ITS chunk).  In occlusion
mode the gathered bytes per second follow from the pairs that reach the depth gather (4 bytes each) under each bound.

    python tests/tools/cull_bench.py --out profiles/cull_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o cull -- python tests/tools/cull_bench.py --trace-run   # -> profiles/cull_kernel_stats.csv
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

from vmap_amd import meshing, visibility  # noqa: E402
from vmap_amd.trainer import SimpleConfig, Trainer  # noqa: E402

W, H = 1200, 680
INTRINSICS = (600.0, 600.0, 599.5, 339.5)
EPS = 0.02
CHUNK = 32                                 # vc::kFrameChunk
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


def scene_mesh(dim):
    """A Trainer.meshing mesh of an untrained hidden-32 field whose head bias is moved so that the 0.5 level has a surface (as
    tests/tools/mesh_bench.py does); a gyroid through extract_mesh if the field has none."""
    bound = meshing.BoundingBox(center=np.array([0.1, 0.2, -0.3]), R=np.eye(3), extent=np.array([1.2, 0.9, 1.0]))
    torch.manual_seed(0)
    tr = Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=32, obj_id=1))
    with torch.no_grad():
        pts = meshing.grid_points((32,) * 3, meshing.bound_affine(bound, tr.bound_extent, 32, torch.tensor(0.0)))
        alpha, _ = tr.fc_occ_map(tr.pe(pts))
        tr.fc_occ_map.out_alpha.bias -= alpha.median() / 10.0
    m = tr.meshing(bound, torch.tensor(0.0), dim)
    if m is not None and len(m.faces) >= 100000:
        return m, "Trainer.meshing, untrained hidden-32 field"
    t = torch.linspace(-1, 1, dim, device=DEV) * 9.0
    X, Y, Z = torch.meshgrid(t, t, t, indexing="ij")
    vol = torch.sigmoid(4 * (torch.sin(X) * torch.cos(Y) + torch.sin(Y) * torch.cos(Z) + torch.sin(Z) * torch.cos(X)))
    return meshing.extract_mesh(vol, 0.5, meshing.bound_affine(bound, tr.bound_extent, dim)), "gyroid through extract_mesh"


def ring_poses(K, centre, radius=2.5):
    t_wc = np.zeros((K, 4, 4), np.float32)
    for k in range(K):
        ang = 2 * np.pi * k / K
        eye = centre + np.array([radius * np.cos(ang), 0.5 * np.sin(2 * ang), radius * np.sin(ang)])
        zc = (centre - eye) / np.linalg.norm(centre - eye)
        xc = np.cross([0.0, 1.0, 0.0], zc)
        xc /= np.linalg.norm(xc)
        t_wc[k, :3, :3], t_wc[k, :3, 3], t_wc[k, 3, 3] = np.stack([xc, np.cross(zc, xc), zc], 1), eye, 1.0
    return torch.from_numpy(t_wc).to(DEV)


def _fma(a, b, c, exact):
    return (a.double() * b.double() + c.double()).float() if exact else a * b + c


def eager_frame(p, T, depth, eps, exact):
    """(seen by this frame bool [n], reaches the depth gather bool [n]): the contract with [n] intermediates.  T: float32 [16]."""
    fx, fy, cx, cy = (torch.tensor(x, dtype=torch.float32, device=p.device) for x in INTRINSICS)
    q0, q1, q2 = p[:, 0] - T[3], p[:, 1] - T[7], p[:, 2] - T[11]
    c = [_fma(q2, T[8 + i], _fma(q1, T[4 + i], q0 * T[i], exact), exact) for i in range(3)]
    z = c[2]
    u, v = _fma(c[0] / z, fx, cx, exact), _fma(c[1] / z, fy, cy, exact)
    w, h = torch.round(u), torch.round(v)                     # half to even
    inside = (z > 0) & (w >= 0) & (w <= W - 1) & (h >= 0) & (h <= H - 1)
    if eps is None:
        return inside, inside
    idx = torch.where(inside, w, torch.zeros_like(w)).long() * H + torch.where(inside, h, torch.zeros_like(h)).long()
    d = depth.reshape(-1)[idx]
    return inside & (d > 0) & (z <= d + eps), inside


def eager_mark(p, images, t_wc, eps, exact=True, census=None):
    """uint8 [n].  ``census``: a dict that receives the evaluated / gathering pair counts under both early-exit bounds."""
    seen = torch.zeros(len(p), dtype=torch.bool, device=p.device)
    t16 = t_wc.reshape(-1, 16)
    if census is not None:
        tot = {k: torch.zeros((), dtype=torch.int64, device=p.device) for k in ("eval_lower", "eval_upper", "gather_lower", "gather_upper")}
    for k in range(len(t16)):
        ok, inside = eager_frame(p, t16[k], None if eps is None else images[k], eps, exact)
        if census is not None:
            if k % CHUNK == 0:
                in_chunk = torch.zeros_like(seen)
            # lower: everything seen so far is known; upper: only what this chunk's own workgroup found (the caller's mask is zero)
            open_lower, open_upper = ~seen, ~in_chunk
            tot["eval_lower"] += open_lower.sum()
            tot["eval_upper"] += open_upper.sum()
            tot["gather_lower"] += (open_lower & inside).sum()
            tot["gather_upper"] += (open_upper & inside).sum()
            in_chunk |= ok
        seen |= ok
    if census is not None:
        census.update({k: int(v) for k, v in tot.items()})
    return seen.to(torch.uint8)


def z_buffer(p, t_wc):
    """float32 [K, W, H]: per frame the smallest z of the vertices that project to each pixel, 0 where none does."""
    depth = torch.zeros(len(t_wc), W * H, dtype=torch.float32, device=p.device)
    fx, fy, cx, cy = INTRINSICS
    for k in range(len(t_wc)):
        c = (p - t_wc[k, :3, 3]) @ t_wc[k, :3, :3]
        z = c[:, 2]
        w, h = torch.round(fx * c[:, 0] / z + cx), torch.round(fy * c[:, 1] / z + cy)
        ok = (z > 0) & (w >= 0) & (w <= W - 1) & (h >= 0) & (h <= H - 1)
        idx = (w[ok].long() * H + h[ok].long())
        buf = torch.full((W * H,), float("inf"), device=p.device)
        buf.scatter_reduce_(0, idx, z[ok], "amin")
        depth[k] = torch.where(torch.isinf(buf), torch.zeros_like(buf), buf)
    return depth.reshape(len(t_wc), W, H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[20, 200])
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true", help="the kernels alone, a few calls each: for rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    mesh, source = scene_mesh(args.dim)
    p = mesh.vertices.contiguous()
    centre = ((p.min(0).values + p.max(0).values) / 2).cpu().numpy().astype(np.float64)
    results = {"device": torch.cuda.get_device_name(0), "mesh": source, "grid": args.dim, "vertices": len(p), "faces": len(mesh.faces),
               "image": [W, H], "occlusion_eps": EPS, "reps": args.reps, "frame_chunk": CHUNK, "runs": []}
    for K in ([20] if args.trace_run else args.frames):
        t_wc = ring_poses(K, centre)
        depth = z_buffer(p, t_wc)
        # "occlusion_none_seen": the same vertices against depth images that measured 0.5 m wherever they measured anything - in front
        # of every vertex, so nothing is seen, no early exit helps and every pair inside a frustum gathers a depth: all the work
        near = torch.where(depth > 0, torch.full_like(depth, 0.5), depth)
        for mode, eps in (("occlusion", EPS), ("frustum", None), ("occlusion_none_seen", EPS)):
            images = near if mode == "occlusion_none_seen" else depth
            mark = lambda: visibility.mark_visible(p, images if eps is not None else None, t_wc, INTRINSICS, eps, size=(W, H))
            seen = mark()
            if args.trace_run:
                for _ in range(3):
                    mark()
                    if mode != "occlusion_none_seen":
                        visibility.cull_mesh(mesh, seen, 1)
                continue
            census = {}
            want = eager_mark(p, images, t_wc, eps, True, census)
            equal = bool(torch.equal(seen, want))
            plain = eager_mark(p, images, t_wc, eps, False)
            pairs = len(p) * K
            rec = {"frames": K, "mode": mode, "seen_share": float(seen.float().mean()), "eager_flags_equal": equal,
                   "plain_float32_eager_differing_flags": int((plain != seen).sum()),
                   "mark_visible_ms": timed(mark, args.reps),
                   "eager_exact_ms": timed(lambda: eager_mark(p, images, t_wc, eps, True), max(2, args.reps // 3)),
                   "eager_plain_float32_ms": timed(lambda: eager_mark(p, images, t_wc, eps, False), max(2, args.reps // 3)),
                   "pairs": pairs, "share_lower": census["eval_lower"] / pairs, "share_upper": census["eval_upper"] / pairs}
            rec["speedup_over_eager_exact"] = rec["eager_exact_ms"] / rec["mark_visible_ms"]
            rec["speedup_over_eager_plain"] = rec["eager_plain_float32_ms"] / rec["mark_visible_ms"]
            rec["pairs_per_s_if_all_evaluated"] = pairs / (rec["mark_visible_ms"] * 1e-3)
            if eps is not None:
                rec["gathered_Bps_lower"] = 4 * census["gather_lower"] / (rec["mark_visible_ms"] * 1e-3)
                rec["gathered_Bps_upper"] = 4 * census["gather_upper"] / (rec["mark_visible_ms"] * 1e-3)
            for min_seen in (1, 3) if mode != "occlusion_none_seen" else ():
                culled = visibility.cull_mesh(mesh, seen, min_seen)
                rec[f"cull_mesh_min_seen_{min_seen}_ms"] = timed(lambda: visibility.cull_mesh(mesh, seen, min_seen), args.reps)
                rec[f"kept_faces_min_seen_{min_seen}"] = 0 if culled is None else len(culled.faces)
            if not equal:
                rec["differing_flags"] = int((want != seen).sum())
            results["runs"].append(rec)
            print(json.dumps(rec), flush=True)
        del depth, near
        torch.cuda.empty_cache()
    if args.out and not args.trace_run:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    if not args.trace_run and not all(r["eager_flags_equal"] for r in results["runs"]):
        sys.exit("the eager baseline's flags differ from the kernel's")


if __name__ == "__main__":
    main()
