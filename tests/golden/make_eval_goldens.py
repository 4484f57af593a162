"""Generate the nearest-neighbour fixtures tests/golden/eval_*.npz with scipy (the reference's metric/metrics.py queries
scipy.spatial.cKDTree).

Run under an interpreter that has scipy (the tests never need it to read the .npz files):
    python tests/golden/make_eval_goldens.py
Each file holds float32 clouds ``gt`` and ``rec`` and what the reference computes from them in float64: cKDTree distances and
indices in both directions (``d_rec_gt`` / ``i_rec_gt``: rec queried against gt; ``d_gt_rec`` / ``i_gt_rec``: gt against rec) and
the metrics ``metrics`` = [accuracy, completion, completion ratio < 0.01, completion ratio < 0.05] (eval_3D_obj.py:37-41 order).
"""
from __future__ import annotations

import os

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))


def _clouds():
    rng = np.random.default_rng(2024)
    # 2k x 3k uniform in a 1 m cube
    yield "uniform", rng.uniform(-0.5, 0.5, (3000, 3)), rng.uniform(-0.5, 0.5, (2000, 3))
    # clustered: 20 blobs of a few cm, rec a noisy copy of gt
    c = rng.uniform(-1, 1, (20, 3))
    gt = c[rng.integers(0, 20, 2500)] + rng.normal(0, 0.03, (2500, 3))
    yield "clustered", gt, gt[rng.integers(0, 2500, 1800)] + rng.normal(0, 0.01, (1800, 3))
    # duplicates in both clouds (ties: the smallest index wins in cKDTree and in the kernel)
    base = rng.uniform(0, 0.3, (400, 3))
    yield "duplicates", np.concatenate([base, base[:200], base[::3]]), np.concatenate([base[::2], base[:50], rng.uniform(0, 0.3, (300, 3))])
    # room scale: a surface-like cloud ~5 m from the origin, rec within a few cm of it
    t = rng.uniform(0, 1, (3000, 2))
    gt = np.stack([5.0 + 2.0 * t[:, 0], -4.0 + 1.5 * t[:, 1], 2.5 + 0.05 * np.sin(9 * t[:, 0])], 1)
    yield "room5m", gt, gt[rng.integers(0, 3000, 2000)] + rng.normal(0, 0.02, (2000, 3))


def main():
    for name, gt, rec in _clouds():
        gt = np.asarray(gt, np.float32)
        rec = np.asarray(rec, np.float32)
        g64, r64 = gt.astype(np.float64), rec.astype(np.float64)
        d_rg, i_rg = cKDTree(g64).query(r64)
        d_gr, i_gr = cKDTree(r64).query(g64)
        m = np.array([d_rg.mean(), d_gr.mean(), (d_gr < 0.01).mean(), (d_gr < 0.05).mean()])
        np.savez_compressed(os.path.join(HERE, f"eval_{name}.npz"), gt=gt, rec=rec, d_rec_gt=d_rg, i_rec_gt=i_rg.astype(np.int64),
                            d_gt_rec=d_gr, i_gt_rec=i_gr.astype(np.int64), metrics=m)
        print(name, gt.shape, rec.shape, m)


if __name__ == "__main__":
    main()
