"""CPU checker of the marching-cubes kernels (vmap_amd/csrc/mesh_kernels.h): the same algorithm, triangle table, output order and
normal formula in plain numpy, written for clarity rather than speed.  It is what tests/test_gpu_mesh.py compares the device output against, and
tests/test_mesh.py checks it against scikit-image's method='lorensen' on the fixtures of tests/golden/mesh_*.npz.

Conventions (the contract of vmapstep_mesh_count / _emit, include/vmapstep.h):
- a corner is above the level iff value > level; a grid edge crosses iff exactly one of its ends is above;
- the crossing on the edge p0 -> p1 (p1 = p0 + e_axis) lies at p0 + t e_axis, t = (level - v0) / (v1 - v0) in float32;
- vertices are ordered by the owning (lower) point's linear index (i * ny + j) * nz + k, then by axis 0, 1, 2;
- faces by cell (its lowest corner's linear index), then by the classic table's order; degenerate triangles are kept;
- normal: numpy.gradient's stencil (central differences, one-sided at the borders) at both ends of the edge, interpolated with t,
  negated (towards decreasing values), mapped by the inverse transpose of the output affine's linear part and normalised
  (a zero vector stays zero).
"""
from __future__ import annotations

import os
import re

import numpy as np

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vmap_amd", "csrc", "mesh_kernels.h")

# corner c -> (di, dj, dk); edge e -> (corner, corner)   (mesh_kernels.h)
CORNERS = np.array([(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0)], np.int64)
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def _edge_owner_axis():
    own, axis = [], []
    for a, b in EDGES:
        d = CORNERS[b] - CORNERS[a]
        ax = int(np.flatnonzero(d)[0])
        own.append(CORNERS[a] if d[ax] > 0 else CORNERS[b])
        axis.append(ax)
    return np.array(own, np.int64), np.array(axis, np.int64)


EDGE_OWNER, EDGE_AXIS = _edge_owner_axis()


def triangle_table():
    """[256][16] int8 edge ids, -1 terminated: the rows of mesh_kernels.h's kMcTri."""
    src = open(_HEADER).read()
    body = src[src.index("kMcTri[256][16] = {"):]
    body = body[body.index("{") + 1:body.index("};")]
    rows = re.findall(r"\{([-0-9,\s]+)\}", body)
    tab = np.array([[int(x) for x in r.split(",")] for r in rows], np.int8)
    assert tab.shape == (256, 16)
    return tab


TABLE = triangle_table()
TRI_COUNT = (TABLE >= 0).sum(1) // 3


def gradient(vol):
    """numpy.gradient of a float32 volume, as [nx, ny, nz, 3] float32 (central differences, one-sided first order at the borders)."""
    return np.stack(np.gradient(np.asarray(vol, np.float32)), -1).astype(np.float32)


def marching_cubes(vol, level=0.5, affine=None):
    """-> (vertices [V,3] float32, faces [F,3] int32, normals [V,3] float32, edge_ids [V] int64 = point * 3 + axis).
    affine: optional [3,4] (linear part | translation) applied to the index-space vertices (float64 here)."""
    vol = np.ascontiguousarray(vol, np.float32)
    nx, ny, nz = vol.shape
    lev = np.float32(level)
    above = vol > lev
    cross = np.zeros(vol.shape + (3,), bool)
    cross[:-1, :, :, 0] = above[:-1] != above[1:]
    cross[:, :-1, :, 1] = above[:, :-1] != above[:, 1:]
    cross[:, :, :-1, 2] = above[:, :, :-1] != above[:, :, 1:]
    flat = cross.reshape(-1)
    edge_ids = np.flatnonzero(flat)                       # point * 3 + axis, already in output order
    vid_of_edge = np.full(flat.size, -1, np.int64)
    vid_of_edge[edge_ids] = np.arange(edge_ids.size)
    pt, ax = edge_ids // 3, edge_ids % 3
    idx = np.stack(np.unravel_index(pt, vol.shape), -1)
    idx1 = idx.copy()
    idx1[np.arange(len(idx1)), ax] += 1
    v0 = vol[tuple(idx.T)]
    v1 = vol[tuple(idx1.T)]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((lev - v0) / (v1 - v0)).astype(np.float32)
    pos = idx.astype(np.float32)
    pos[np.arange(len(pos)), ax] += t
    g = gradient(vol)
    tt = t[:, None]
    nrm = -(g[tuple(idx.T)] * (np.float32(1) - tt) + g[tuple(idx1.T)] * tt)

    # faces: cells by linear index of their lowest corner, triangles in table order
    if min(vol.shape) >= 2:
        cube = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
        for c, (di, dj, dk) in enumerate(CORNERS):
            cube |= above[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk].astype(np.int64) << c
        cells = np.flatnonzero(TRI_COUNT[cube.reshape(-1)] > 0)
    else:
        cube, cells = np.zeros((0, 0, 0), np.int64), np.zeros(0, np.int64)
    cidx = np.stack(np.unravel_index(cells, cube.shape), -1) if cells.size else np.zeros((0, 3), np.int64)
    ccube = cube.reshape(-1)[cells]
    tris = TABLE[ccube].astype(np.int64)                   # [C,16]
    faces = []
    for s in range(5):
        e = tris[:, 3 * s:3 * s + 3]
        ok = e[:, 0] >= 0
        if not ok.any():
            continue
        owner = cidx[ok][:, None, :] + EDGE_OWNER[e[ok]]  # [c,3,3]
        opt = (owner[..., 0] * ny + owner[..., 1]) * nz + owner[..., 2]
        v = vid_of_edge[opt * 3 + EDGE_AXIS[e[ok]]]
        assert (v >= 0).all()
        faces.append((cells[ok] * 8 + s, v))
    if faces:
        key = np.concatenate([k for k, _ in faces])
        f = np.concatenate([v for _, v in faces])[np.argsort(key, kind="stable")].astype(np.int32)
    else:
        f = np.zeros((0, 3), np.int32)

    if affine is not None:
        A = np.asarray(affine, np.float64).reshape(3, 4)
        pos = (pos.astype(np.float64) @ A[:, :3].T + A[:, 3]).astype(np.float32)
        nrm = (nrm.astype(np.float64) @ np.linalg.inv(A[:, :3])).astype(np.float32)     # (A^-T n) as rows
    nn = np.sqrt((nrm.astype(np.float64) ** 2).sum(1, keepdims=True))
    nrm = np.where(nn > 0, nrm / np.where(nn > 0, nn, 1), 0).astype(np.float32)
    return pos, f, nrm, edge_ids


def canonical_faces(faces, edge_ids):
    """Faces as edge-id triples, each rotated so its smallest id comes first (winding kept), rows sorted: for comparing meshes
    whose vertex order differs."""
    e = np.asarray(edge_ids, np.int64)[np.asarray(faces, np.int64)]
    r = np.argmin(e, 1)
    rows = np.arange(len(e))
    out = np.stack([e[rows, r], e[rows, (r + 1) % 3], e[rows, (r + 2) % 3]], 1)
    return out[np.lexsort(out.T[::-1])] if len(out) else out.reshape(0, 3)


def vertex_edge_ids(vertices, shape):
    """Map index-space vertices (each inside a grid edge) to point * 3 + axis; -1 where a vertex does not have exactly one
    non-integer coordinate (a vertex at a grid point, t = 0 or 1, or Lewiner's vertex inside a cell)."""
    v = np.asarray(vertices, np.float64)
    fl = np.floor(v)
    frac = v - fl
    nonint = frac > 1e-6
    ax = np.argmax(nonint, 1)
    base = fl.astype(np.int64)
    pt = np.ravel_multi_index(tuple(np.clip(base, 0, np.array(shape) - 1).T), shape)
    ids = pt * 3 + ax
    ids[nonint.sum(1) != 1] = -1
    return ids
