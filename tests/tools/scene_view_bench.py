"""Scene view at Replica frame size: 1200 x 680, the 20 hidden-32 objects of view_bench.py at S = 16 plus a hidden-128 field (the
background model's width) in a room box around the camera at S = 48 (device events around each call, one warm-up, median and spread of
--reps; the legs that are compared are alternated in rounds).

Reported: ms per scene render (render_view_groups as the user calls it: count, the host read of the offsets, emit, both packs, both
field kernels, composite); ms for the background group alone (render_view at hidden 128); and the render call of the background group
without the count (vmapstep_scene_view_render alone: emit + pack + field_query_seg_gen<4> + composite) next to Trainer.eval_points at
hidden 128 (pack + field_query_gen<4>) on as many materialised points, alternated, both as samples per second and as the share of the
float32 matrix peak (2 H (4 H + 220) FLOP per sample, 157 TFLOP/s).  Per-kernel times come from a kernel trace of --trace-run:

    python tests/tools/scene_view_bench.py --out profiles/scene_view_bench.json
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/tools/scene_view_bench.py --trace-run   # -> profiles/scene_view_kernel_stats.csv
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import view_bench as vb  # noqa: E402
from vmap_amd import _devmem, _lib, render, synth  # noqa: E402
from vmap_amd.meshing import BoundingBox  # noqa: E402
from vmap_amd.trainer import SimpleConfig, Trainer  # noqa: E402

W, H, K4, MIN_DEPTH, DEV = vb.W, vb.H, vb.K4, vb.MIN_DEPTH, vb.DEV
S_OBJ, S_BG, H_BG = vb.S, 48, 128
PEAK_F32_MATRIX = 157e12
FLOP_PER_SAMPLE = 2 * H_BG * (4 * H_BG + 220)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true", help="three scene renders and three point queries only: the run to put under a kernel trace")
    a = ap.parse_args()
    fields, boxes, T, centers = vb.scene()
    room = BoundingBox(center=np.array([0.0, 0.0, 0.5], np.float32), R=np.eye(3, dtype=np.float32), extent=np.array([8.0, 8.0, 6.0], np.float32))
    fc, B, sc = synth.make_params(1, H_BG, seed=6)
    bg = ([torch.from_numpy(x).to(DEV) for x in fc], torch.from_numpy(B).to(DEV), torch.from_numpy(sc).to(DEV))
    groups = [render.FieldGroup(fields, boxes, centers, S_OBJ), render.FieldGroup(bg, [room], None, S_BG)]
    kw = dict(min_depth=MIN_DEPTH, budget_bytes=1 << 40)
    scene = lambda: render.render_view_groups(groups, T, K4, W, H, **kw)
    alone = lambda: render.render_view(bg, [room], T, K4, W, H, samples=S_BG, **kw)
    view = alone()
    n_pts = view.n_pairs * S_BG
    tr = Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=H_BG, obj_scale=2.0))
    pts = (torch.rand(n_pts, 3, device=DEV) - 0.5)
    if a.trace_run:
        for _ in range(3):
            scene()
            tr._eval_points_hip(pts)
        torch.cuda.synchronize()
        return
    whole = scene()
    res = {"tool": "scene_view_bench", "width": W, "height": H, "objects": vb.N_OBJ, "object_samples": S_OBJ, "background_hidden": H_BG,
           "background_samples": S_BG, "pairs_per_scene": whole.n_pairs, "background_pairs": view.n_pairs, "background_samples_per_view": n_pts,
           "overflow_pixels": whole.overflow, "device": torch.cuda.get_device_name(0)}
    rounds = {"render_view_groups": [], "background_group_alone": []}
    for _ in range(3):
        rounds["render_view_groups"].append(vb.timed(scene, a.reps))
        rounds["background_group_alone"].append(vb.timed(alone, a.reps))
    for k, v in rounds.items():
        med = [r["median_ms"] for r in v]
        res[k] = {"median_ms_per_round": med, "median_ms": statistics.median(med), "spread_over_rounds": (max(med) - min(med)) / statistics.median(med)}
    # the render call of the background group alone against the point query on as many points, alternated
    lib = _lib.load()
    pp = _lib.Params()
    for t, p in enumerate(bg[0]):
        pp.fc[t] = _lib.Tensor(p.data_ptr(), p.stride(0))
    pp.pe_B = _lib.Tensor(bg[1].data_ptr(), bg[1].stride(0))
    scl = _lib.Tensor(bg[2].data_ptr(), 1)
    garr = (_lib.ViewGroup * 1)(_lib.ViewGroup(H_BG, 1, S_BG, 0, ctypes.pointer(pp), ctypes.pointer(scl)))
    cfg = _lib.ViewCfg(W, H, 0, 1, *K4, (ctypes.c_float * 16)(*T.reshape(-1)), MIN_DEPTH, 0, W * H)
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_scene_view_workspace_bytes, DEV, ctypes.byref(cfg), garr, 1)
    boxes_d = torch.from_numpy(render._box_rows([room], 1)).to(DEV)
    centers_d = torch.zeros(1, 3, device=DEV)
    off_d = torch.empty(2, dtype=torch.int64, device=DEV)
    _lib.check(lib.vmapstep_scene_view_count(ctypes.byref(cfg), garr, 1, boxes_d.data_ptr(), off_d.data_ptr(), ws_ptr, nbytes, _devmem.stream(DEV)), lib)
    off_h = off_d.cpu().numpy().copy()
    m = int(off_h[-1])
    bufs = [torch.empty(m, 4, dtype=torch.int32, device=DEV), torch.empty(m * S_BG, device=DEV), torch.empty(m * S_BG, 3, device=DEV), torch.empty(W, H, device=DEV),
            torch.empty(W, H, 3, device=DEV), torch.empty(W, H, device=DEV), torch.empty(W, H, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)]

    def call_render():
        _lib.check(lib.vmapstep_scene_view_render(ctypes.byref(cfg), garr, 1, boxes_d.data_ptr(), centers_d.data_ptr(), off_d.data_ptr(),
                                                  off_h.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), bufs[0].data_ptr(), m,
                                                  *(b.data_ptr() for b in bufs[1:]), ws_ptr, nbytes, _devmem.stream(DEV)), lib)

    rounds = {"scene_view_render_call": [], "eval_points_call": []}
    for _ in range(3):                                             # alternated: each leg sees the same machine state
        rounds["scene_view_render_call"].append(vb.timed(call_render, a.reps))
        rounds["eval_points_call"].append(vb.timed(lambda: tr._eval_points_hip(pts), a.reps))
    for k, v in rounds.items():
        med = [r["median_ms"] for r in v]
        ms = statistics.median(med)
        res[k] = {"median_ms_per_round": med, "samples_per_s": n_pts / (ms * 1e-3), "spread_over_rounds": (max(med) - min(med)) / ms,
                  "share_of_f32_matrix_peak": n_pts * FLOP_PER_SAMPLE / (ms * 1e-3) / PEAK_F32_MATRIX}
    res["bound_ms_at_f32_matrix_peak"] = n_pts * FLOP_PER_SAMPLE / PEAK_F32_MATRIX * 1e3
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
