"""TSDF fusion at scene size: a 256^3 volume over the box of the bench scene (the analytic room corner with a sphere of
tests/icp_cases.py, ray-cast on the device at 1200 x 680 from 20 poses on an arc looking inward), with and without colour, for the
whole scene and for one object (the sphere, its own box).  Time per ``integrate`` (all 20 frames in one call: device events around
the call, median of --reps, warm), per frame, and per ``extract_mesh``; the same with one frame per call, which is what taking frames
in batches saves.

Roofline.  One call must read and write the volume once: 16 bytes per voxel (D, W in and out), 48 with colour.  The yardstick is a
device-to-device copy that moves the same bytes (``copy_`` of half of them: a copy reads and writes each), timed the same way.  The
JSON says which side of it the kernel sits on; the kernel also projects every voxel into every frame (about 40 float operations and a
division pair per pair) and gathers depth for the pairs inside a frustum, so it can only match the copy when that work hides under the
volume's traffic.  Whether it does is what the JSON records (``integrate_over_copy``, ``side_of_the_roofline``).  A copy of less than
256 MB is partly served by the Infinity Cache: the yardstick flatters the copy there, never the kernel.

Eager torch path of the same contract in the same process on the same inputs: frame by frame with [n] intermediates, every fused
multiply-add through a float64 product and sum.  Its agreement with the kernel (voxels whose bits differ, largest difference) is
recorded; it is not the kernel's test - tests/test_gpu_tsdf.py holds the kernel to the exact checker.

    python tests/tools/tsdf_bench.py --out profiles/tsdf_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o tsdf -- python tests/tools/tsdf_bench.py --trace-run   # -> profiles/tsdf_kernel_stats.csv
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import icp_cases as ic  # noqa: E402
from vmap_amd import meshing, tsdf  # noqa: E402

W, H, K = 1200, 680, 20
INTRINSICS = ic.intrinsics_for(W, H)
DIM = 256
SCENE_LO, SCENE_HI = -0.1, 2.46                    # 1 cm voxels at 256^3
MAX_DEPTH = 10.0
SPHERE_ID, WALL_ID = 1, 2
DEV = "cuda:0"


def timed(fn, reps, before=None):
    """Median device time (ms) of fn over reps calls after one warm call, events around each call on the current stream."""
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


def render(t_wc):
    """icp_cases.render on the device, float64: (depth float32 [W, H], inst int32 [W, H])."""
    fx, fy, cx, cy = INTRINSICS
    T = torch.as_tensor(t_wc, dtype=torch.float64, device=DEV)
    w, h = torch.meshgrid(torch.arange(W, dtype=torch.float64, device=DEV), torch.arange(H, dtype=torch.float64, device=DEV), indexing="ij")
    d = torch.stack([(w - cx) / fx, (h - cy) / fy, torch.ones_like(w)], -1) @ T[:3, :3].T
    o = T[:3, 3]
    best = torch.full((W, H), float("inf"), dtype=torch.float64, device=DEV)
    for k in range(3):
        t = -o[k] / d[..., k]
        hit = o + t[..., None] * d
        ok = (t > 0) & (hit >= -1e-9).all(-1)
        best = torch.where(ok & (t < best), t, best)
    walls = best.clone()
    oc = o - torch.as_tensor(ic.SPHERE_CENTER, dtype=torch.float64, device=DEV)
    a, b, c = (d * d).sum(-1), 2 * (d * oc).sum(-1), oc @ oc - ic.SPHERE_RADIUS ** 2
    disc = b * b - 4 * a * c
    t = (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a)
    sphere = (disc > 0) & (t > 0) & (t < best)
    best = torch.where(sphere, t, best)
    inst = torch.where(sphere, SPHERE_ID, torch.where(torch.isfinite(walls), WALL_ID, -1)).to(torch.int32)
    return torch.where(torch.isfinite(best), best, torch.zeros_like(best)).float(), inst


def frames():
    eyes = [(1.9 + 0.9 * np.cos(a), 1.9 + 0.9 * np.sin(a), 1.3 + 0.4 * np.sin(3 * a)) for a in np.linspace(-0.3, 1.9, K)]
    t_wc = np.stack([ic.look_at(e, (0.45, 0.5, 0.4)) for e in eyes]).astype(np.float32)
    pairs = [render(T) for T in t_wc]
    depth, inst = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    w, h = torch.meshgrid(torch.arange(W, device=DEV), torch.arange(H, device=DEV), indexing="ij")
    rgbx = torch.stack([torch.stack([(7 * w + 3 * h + 40 * k) % 256, (5 * h + 11 * k) % 256, (w * h + k) % 256, 0 * w], -1) for k in range(K)]).to(torch.uint8)
    return depth.contiguous(), inst.contiguous(), rgbx.contiguous(), torch.from_numpy(t_wc).to(DEV)


def volume(which, color):
    if which == "scene":
        s = (SCENE_HI - SCENE_LO) / (DIM - 1)
        A = np.array([[s, 0, 0, SCENE_LO], [0, s, 0, SCENE_LO], [0, 0, s, SCENE_LO]])
    else:
        box = meshing.BoundingBox(center=ic.SPHERE_CENTER, R=np.eye(3), extent=np.full(3, 2 * ic.SPHERE_RADIUS + 0.1))
        A = meshing.bound_affine(box, 1.0, DIM)
    voxel = float(np.linalg.norm(np.asarray(A)[:, 0]))
    return tsdf.TSDFVolume((DIM,) * 3, A, 4 * voxel, color=color, device=DEV), voxel


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def eager_integrate(vol, depth, inst, rgbx, t_wc, obj_id):
    """The contract in eager torch, frame by frame: (D, W, C) as new tensors."""
    fx, fy, cx, cy = INTRINSICS
    n = vol.tsdf.numel()
    p = meshing.grid_points(vol.shape, vol.affine, DEV)
    D, Wt = vol.tsdf.reshape(-1).clone(), vol.weight.reshape(-1).clone()
    C = None if vol.color is None else vol.color.clone()
    tr, mw = vol.trunc, vol.max_weight
    for k in range(len(t_wc)):
        T = t_wc[k].reshape(-1)
        q0, q1, q2 = p[:, 0] - T[3], p[:, 1] - T[7], p[:, 2] - T[11]
        c = [fma(T[8 + i], q2, fma(T[4 + i], q1, T[i] * q0)) for i in range(3)]
        z = c[2]
        u, v = fma(torch.tensor(fx, device=DEV), c[0] / z, torch.tensor(cx, device=DEV)), fma(torch.tensor(fy, device=DEV), c[1] / z, torch.tensor(cy, device=DEV))
        w, h = torch.round(u), torch.round(v)
        ok = (z > 0) & (w >= 0) & (w <= W - 1) & (h >= 0) & (h <= H - 1)
        pix = torch.where(ok, w * H + h, torch.zeros_like(w)).long()
        d = depth[k].reshape(-1)[pix]
        ok &= (d > 0) & (d <= MAX_DEPTH)
        if obj_id is not None:
            ok &= inst[k].reshape(-1)[pix] == obj_id
        sdf = d - z
        ok &= sdf >= -tr
        s = torch.clamp_max(sdf / tr, 1.0)
        W1 = Wt + 1
        D = torch.where(ok, fma(D, Wt, s) / W1, D)
        if C is not None:
            band = ok & (sdf <= tr)
            wc = C[:, 3].clone()
            wc1 = wc + 1
            px = rgbx[k].reshape(-1, 4)[pix].float()
            for ch in range(3):
                C[:, ch] = torch.where(band, fma(C[:, ch], wc, px[:, ch]) / wc1, C[:, ch])
            C[:, 3] = torch.where(band, torch.clamp_max(wc1, mw), wc)
        Wt = torch.where(ok, torch.clamp_max(W1, mw), Wt)
    assert n == D.numel()
    return D, Wt, C


def agreement(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    differ = a.view(torch.int32) != b.view(torch.int32)
    return {"values": int(a.numel()), "bits_differ": int(differ.sum()), "max_abs_difference": float((a - b).abs().max())}


def run_case(which, color, data, reps, eager):
    depth, inst, rgbx, t_wc = data
    obj_id = SPHERE_ID if which == "object" else None
    vol, voxel = volume(which, color)
    kw = dict(rgb=rgbx if color else None, inst=inst if obj_id is not None else None, obj_id=obj_id, max_depth=MAX_DEPTH)
    n = vol.tsdf.numel()
    ms_all = timed(lambda: vol.integrate(depth, t_wc, INTRINSICS, **kw), reps, before=vol.reset)

    def one_by_one():
        for k in range(K):
            vol.integrate(depth, t_wc, INTRINSICS, slots=[k], **kw)
    ms_single = timed(one_by_one, max(1, reps // 3), before=vol.reset)
    vol.reset()
    vol.integrate(depth, t_wc, INTRINSICS, **kw)
    touched = int((vol.weight > 0).sum())
    bytes_min = n * (8 + (16 if color else 0)) + touched * (8 + (16 if color else 0))       # read all, write what changed
    bytes_full = n * (16 + (32 if color else 0))
    src = torch.empty(bytes_full // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    ms_copy = timed(lambda: dst.copy_(src), reps)
    ms_mesh = timed(lambda: vol.extract_mesh(), max(1, reps // 3))
    mesh = vol.extract_mesh()
    out = {"volume": which, "color": color, "obj_id": obj_id, "voxels": n, "voxel_size_m": voxel, "trunc_m": vol.trunc, "frames": K,
           "integrate_ms": ms_all, "integrate_ms_per_frame": ms_all / K, "one_frame_per_call_ms_total": ms_single,
           "one_frame_per_call_ms_per_frame": ms_single / K, "voxels_updated": touched,
           "volume_bytes_read_and_written_every_voxel": bytes_full, "volume_bytes_read_all_written_updated": bytes_min,
           "device_copy_of_the_same_bytes_ms": ms_copy, "integrate_over_copy": ms_all / ms_copy,
           "side_of_the_roofline": "above the copy: bound by projection arithmetic and depth gathers, not by the volume's traffic"
           if ms_all > ms_copy else "at the copy: bound by the volume's traffic",
           "pairs_per_second": n * K / (ms_all * 1e-3),
           "extract_mesh_ms": ms_mesh, "mesh_vertices": 0 if mesh is None else len(mesh.vertices), "mesh_faces": 0 if mesh is None else len(mesh.faces)}
    if eager:
        ref = type(vol)(vol.shape, vol.affine, vol.trunc, color=color, device=DEV)
        ms_eager = timed(lambda: eager_integrate(ref, depth, inst, rgbx, t_wc, obj_id), 1)
        D, Wt, C = eager_integrate(ref, depth, inst, rgbx, t_wc, obj_id)
        out.update({"eager_torch_ms": ms_eager, "eager_over_kernel": ms_eager / ms_all,
                    "agreement_with_eager_torch": {"tsdf": agreement(vol.tsdf, D), "weight": agreement(vol.weight, Wt),
                                                   **({"color": agreement(vol.color, C)} if color else {})}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-eager", action="store_true", help="skip the eager torch path (A/B runs of kernel forms)")
    ap.add_argument("--trace-run", action="store_true", help="a few calls of every kernel and nothing else, for a rocprofv3 kernel trace")
    args = ap.parse_args()
    data = frames()
    if args.trace_run:
        for which in ("scene", "object"):
            for color in (False, True):
                run_case(which, color, data, 3, eager=False)
        torch.cuda.synchronize()
        return
    results = [run_case(which, color, data, args.reps, eager=not args.no_eager) for which in ("scene", "object") for color in (False, True)]
    doc = {"tool": "tests/tools/tsdf_bench.py", "device": torch.cuda.get_device_name(0), "image": [W, H], "frames": K, "reps": args.reps,
           "timing": "median of device events around each call, warm", "cases": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
