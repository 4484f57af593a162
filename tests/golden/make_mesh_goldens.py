"""Generate the marching-cubes fixtures tests/golden/mesh_*.npz with scikit-image (the reference's vis.py:6-19 calls
skimage.measure.marching_cubes(occ, level=0.5, gradient_direction='ascent')).

Run only under an interpreter that has scikit-image (the tests never import it; they read the .npz files):
    <python with skimage> tests/golden/make_mesh_goldens.py
Each volume file holds the input ``volume`` and skimage's ``{lorensen,lewiner}_{vertices,faces,normals}`` for level 0.5,
gradient_direction='ascent' (allow_degenerate=True, the defaults otherwise), plus ``lewiner_case``: the Lewiner case number of each
of the 256 cube indices (column 0 of skimage's CASES table: 3, 4, 6, 7, 10, 12 and 13 are the configurations with an ambiguous face
or interior).  ``mesh_transform.npz`` records the reference's transform chain (trainer.py:35-75, render_rays.py:98-122) in float64.
"""
from __future__ import annotations

import base64
import os

import numpy as np
from skimage import measure
from skimage.measure import _marching_cubes_lewiner_luts as luts

HERE = os.path.dirname(os.path.abspath(__file__))


def _grid(shape):
    return np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def volumes():
    X, Y, Z = _grid((32, 32, 32))
    yield "sphere", _sigmoid(10 * (0.6 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)))
    X, Y, Z = _grid((24, 28, 20))
    r = np.sqrt((X * 1.3) ** 2 + Y ** 2 + (Z * 0.8) ** 2) + 0.05 * np.sin(5 * X) * np.cos(3 * Y)
    yield "blob", _sigmoid(10 * (0.6 - r))
    X, Y, Z = _grid((20, 33, 27))
    r = np.sqrt((X * 0.9) ** 2 + (Y * 1.2) ** 2 + Z ** 2) + 0.08 * np.sin(4 * Z + 1) * np.cos(2 * X)
    yield "noncubic", _sigmoid(8 * (0.55 - r))
    # smoothed noise: many ambiguous cells
    rng = np.random.default_rng(1)
    shape = (28, 28, 28)
    g = rng.standard_normal(shape)
    K = np.sqrt(sum(k ** 2 for k in np.meshgrid(*[np.fft.fftfreq(n) * n / 4.0 for n in shape], indexing="ij")))
    o = np.real(np.fft.ifftn(np.fft.fftn(g) * np.exp(-K ** 2)))
    yield "noise", _sigmoid(10 * o / o.std())
    # corner values exactly at the level: a coarse field quantised to multiples of 1/8 (0.5 among them)
    X, Y, Z = _grid((9, 10, 11))
    q = np.round(_sigmoid(4 * (0.5 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2))) * 8) / 8
    yield "exact", q
    yield "tiny", np.array([[[0.2, 0.7], [0.4, 0.3]], [[0.9, 0.1], [0.6, 0.45]]])


def lewiner_case():
    shape, text = luts.CASES
    return np.frombuffer(base64.decodebytes(text.encode("utf-8")), dtype=np.int8).reshape(shape)[:, 0].copy()


def write_volume(name, vol):
    vol = vol.astype(np.float32)
    out = {"volume": vol, "lewiner_case": lewiner_case()}
    for method in ("lorensen", "lewiner"):
        v, f, n, _ = measure.marching_cubes(vol, level=0.5, gradient_direction="ascent", method=method)
        out[f"{method}_vertices"] = v.astype(np.float32)
        out[f"{method}_faces"] = f.astype(np.int32)
        out[f"{method}_normals"] = n.astype(np.float32)
    path = os.path.join(HERE, f"mesh_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {vol.shape}, {len(out['lorensen_vertices'])} vertices, {len(out['lorensen_faces'])} faces (lorensen), "
          f"{len(out['lewiner_faces'])} (lewiner), {os.path.getsize(path)} bytes")


def write_transform():
    """The reference's chain in float64 for a rotated anisotropic bound, an odd D and a non-zero obj_center."""
    D, bound_extent = 17, 0.9
    ang = 0.7
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(-0.4), -np.sin(-0.4)], [0, np.sin(-0.4), np.cos(-0.4)]])
    R = Rz @ Rx
    extent, center, obj_center = np.array([0.8, 1.3, 0.5]), np.array([0.3, -1.1, 2.0]), np.array([0.05, -0.02, 0.1])
    # make_3D_grid (render_rays.py:98-122) + trainer.py:37-49
    scale = extent / (2.0 * bound_extent)
    t = np.linspace(-1.0, 1.0, D)
    g = np.stack(np.meshgrid(t, t, t, indexing="ij"), -1) * scale
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, center
    grid = np.stack([(T[r, :3] * g).sum(-1) for r in range(3)], -1) + T[:3, 3]
    grid = grid.reshape(-1, 3) - obj_center
    # vis.py:16 (v / (D - 1)) + trainer.py:58-64 (translate -0.5, scale 2, scale by scene_scale, apply transform)
    rng = np.random.default_rng(3)
    v_index = rng.uniform(0, D - 1, size=(64, 3))
    v = v_index / (D - 1)
    v = (v - 0.5) * 2 * scale
    v_scene = v @ R.T + center
    path = os.path.join(HERE, "mesh_transform.npz")
    np.savez_compressed(path, D=D, bound_extent=bound_extent, R=R, extent=extent, center=center, obj_center=obj_center,
                        grid=grid, v_index=v_index, v_scene=v_scene)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for name, vol in volumes():
        write_volume(name, vol)
    write_transform()
