"""Mesh components at scene size, three shapes with about the same face count: the 256^3 ``Trainer.meshing`` mesh of the mesh bench
(one giant component plus floaters), as many faces of disjoint tetrahedra (most roots, least contention) and a single fan (every
face on one hub: the worst contention on one root and one statistics row).  Time per ``label_components``, ``component_stats`` and
``keep_components`` (device events around each call, median of --reps, warm) against two yardsticks in the same process on the same
inputs, both REQUIRED to give equal labels: an eager torch path of the same contract (min-label propagation over the faces by
scatter_reduce(amin) with pointer jumping to a fixed point, then bincount) and, where it can be imported, scipy's
connected_components on the host (the time includes building its sparse matrix from host arrays, not the download).
There is no parent-commit time: the capability is new.

With --kernel-stats (the CSV of a rocprofv3 --kernel-trace --stats run of --trace-run, which runs the mesh shape alone) the bytes
comp_hook and the two statistics kernels must move - faces 12 B, parent read and written 8 B per vertex; faces 12 B, labels 4 B and
positions 12 B per vertex, 20 B of output per component - are set against a device-to-device copy of as many bytes timed in this run.

    python tests/tools/components_bench.py --out profiles/components_bench.json [--kernel-stats profiles/components_kernel_stats.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o comp -- python tests/tools/components_bench.py --trace-run
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vmap_amd import components, meshing  # noqa: E402
from cull_bench import scene_mesh, timed  # noqa: E402

DEV = "cuda:0"


def tetrahedra(n_faces):
    count = n_faces // 4
    tf = torch.tensor([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], dtype=torch.int32, device=DEV)
    faces = (tf[None] + 4 * torch.arange(count, dtype=torch.int32, device=DEV)[:, None, None]).reshape(-1, 3)
    return meshing.Mesh(torch.rand(4 * count, 3, device=DEV), faces.contiguous(), None)


def fan(n_faces):
    rim = torch.arange(1, n_faces + 2, dtype=torch.int32, device=DEV)
    faces = torch.stack([torch.zeros(n_faces, dtype=torch.int32, device=DEV), rim[:-1], rim[1:]], 1)
    return meshing.Mesh(torch.rand(n_faces + 2, 3, device=DEV), faces.contiguous(), None)


def eager_labels(mesh):
    """(labels int32 [V], C): every vertex takes the smallest index among its faces' corners, then its label's label, until nothing
    changes (one host read per round); the fixed point is the component's smallest vertex, numbered by a cumulative sum."""
    n = len(mesh.vertices)
    f = mesh.faces.long()
    ok = ((f >= 0) & (f < n)).all(1)
    f = f[ok]
    label = torch.arange(n, device=f.device)
    while True:
        m = label[f].amin(1, keepdim=True).expand(-1, 3).reshape(-1)
        new = label.scatter_reduce(0, f.reshape(-1), m, "amin")
        new = new[new]
        if torch.equal(new, label):
            break
        label = new
    root = label == torch.arange(n, device=f.device)
    dense = torch.cumsum(root, 0) - 1
    return dense[label].to(torch.int32), int(root.sum())


def eager_stats(mesh, labels, C):
    """(vertices, faces, area_q) by bincount; the area in torch's float32 with its own rounding of the square root - compared, not
    required equal."""
    n = len(mesh.vertices)
    f = mesh.faces.long()
    f = f[((f >= 0) & (f < n)).all(1)]
    lab = labels.long()
    p = mesh.vertices
    a, b = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    c0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    c1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    c2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    area = 0.5 * torch.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
    q = torch.round(torch.nan_to_num(area, 0.0, 0.0, 0.0).double() * 2.0 ** 40).long()
    comp = lab[f[:, 0]]
    area_q = torch.zeros(C, dtype=torch.int64, device=p.device).scatter_add_(0, comp, q)
    return torch.bincount(lab, minlength=C), torch.bincount(comp, minlength=C), area_q


def scipy_labels(faces_host, n):
    from scipy import sparse
    from scipy.sparse.csgraph import connected_components
    f = faces_host
    rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    graph = sparse.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n))
    return connected_components(graph, directed=False)


def kernel_stats(path):
    """{kernel name: average ns} of the comp_* kernels from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            for k in ("comp_init", "comp_hook", "comp_flatten", "comp_scan", "comp_root_emit", "comp_relabel", "comp_face_stats", "comp_vertex_stats"):
                if f"vcc::{k}(" in r["Name"]:
                    out[k] = float(r["AverageNs"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of a rocprofv3 run of --trace-run")
    ap.add_argument("--trace-run", action="store_true", help="the mesh shape alone, ten calls of each entry (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    mesh, source = scene_mesh(args.dim)
    mesh = meshing.Mesh(mesh.vertices.contiguous(), mesh.faces.contiguous(), None)
    if args.trace_run:
        for _ in range(10):
            labels, C = components.label_components(mesh)
            components.component_stats(mesh, labels, C)
        torch.cuda.synchronize()
        return
    F = len(mesh.faces)
    shapes = [("mesh", source, mesh), ("tetrahedra", "disjoint tetrahedra", tetrahedra(F)), ("fan", "one fan around vertex 0", fan(F))]
    results = {"device": torch.cuda.get_device_name(0), "grid": args.dim, "reps": args.reps, "runs": []}
    ok = True
    for name, what, m in shapes:
        V, Fm = len(m.vertices), len(m.faces)
        labels, C = components.label_components(m)
        st = components.component_stats(m, labels, C)
        e_labels, e_C = eager_labels(m)
        e_st = eager_stats(m, e_labels, e_C)
        rec = {"shape": name, "what": what, "vertices": V, "faces": Fm, "components": C,
               "largest_component_faces": int(st.faces.max()), "eager_labels_equal": bool(e_C == C and torch.equal(e_labels, labels)),
               "eager_counts_equal": bool(torch.equal(e_st[0], st.vertices.long()) and torch.equal(e_st[1], st.faces)),
               "eager_area_q_differing_rows": int((e_st[2] != st.area_q).sum()),
               "label_components_ms": timed(lambda: components.label_components(m), args.reps),
               "component_stats_ms": timed(lambda: components.component_stats(m, labels, C), args.reps),
               "keep_components_ms": timed(lambda: components.keep_components(m, min_area=1e-4, largest=1), args.reps),
               "eager_labels_ms": timed(lambda: eager_labels(m), max(2, args.reps // 3)),
               "eager_stats_ms": timed(lambda: eager_stats(m, e_labels, e_C), max(2, args.reps // 3))}
        rec["label_speedup_over_eager"] = rec["eager_labels_ms"] / rec["label_components_ms"]
        rec["stats_speedup_over_eager"] = rec["eager_stats_ms"] / rec["component_stats_ms"]
        ok = ok and rec["eager_labels_equal"] and rec["eager_counts_equal"]
        try:
            host = m.faces.cpu().numpy().astype(np.int64)
            t0 = time.perf_counter()
            s_C, s_labels = scipy_labels(host, V)
            rec["scipy_host_ms"] = (time.perf_counter() - t0) * 1e3
            rec["scipy_labels_equal"] = bool(s_C == C and np.array_equal(s_labels, labels.cpu().numpy()))
            ok = ok and rec["scipy_labels_equal"]
        except ImportError:
            rec["scipy_host_ms"] = None
        if name == "mesh":
            # the bytes the kernels must move against a device-to-device copy of as many bytes (read + written = 2 x half)
            need = {"comp_hook": 12 * Fm + 8 * V, "comp_face_stats": 12 * Fm + 16 * V + 16 * C, "comp_vertex_stats": 4 * V + 4 * C}
            ks = kernel_stats(args.kernel_stats) if args.kernel_stats else {}
            rec["kernels"] = {}
            for k, nbytes in need.items():
                half = nbytes // 2
                src, dst = torch.empty(half, dtype=torch.uint8, device=DEV), torch.empty(half, dtype=torch.uint8, device=DEV)
                copy_ms = timed(lambda: dst.copy_(src), args.reps)
                row = {"bytes": nbytes, "copy_ms": copy_ms, "copy_bytes_per_s": 2 * half / (copy_ms * 1e-3)}
                if k in ks:
                    rate = nbytes / (ks[k] * 1e-9)
                    row.update(kernel_us=ks[k] / 1e3, kernel_bytes_per_s=rate, fraction_of_copy_rate=rate / row["copy_bytes_per_s"])
                rec["kernels"][k] = row
            rec["kernel_us"] = {k: v / 1e3 for k, v in sorted(ks.items())}
        results["runs"].append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    if not ok:
        sys.exit("a yardstick's labels or counts differ from the kernels'")


if __name__ == "__main__":
    main()
