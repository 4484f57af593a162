"""Numpy checker of TSDF fusion (vmap_amd/tsdf.py, csrc/tsdf_kernels.h, csrc/tsdf_rules.h) and of marching cubes over observed voxels
(the valid mask of csrc/mesh_kernels.h), written from the contract of the tsdf and mesh sections of include/vmapstep.h, not from the
kernels.  Nothing in it can be held against an outside implementation: the contract is this project's own.  Two layers:

- ``integrate_f32``: the float32 arithmetic of the contract with every fused multiply-add emulated exactly (filter_oracle.fmaf); the
  host program and the device must equal it bit for bit;
- ``integrate_f64``: the same rule in plain float64, no emulation: what the geometry tests measure.

Depth images are [K, W, H], width-major; rgbx [K, W, H, 4] uint8; inst [K, W, H] int32; poses [K, 4, 4] camera to world.  A volume is a
dict: tsdf [n], weight [n] and color [n, 4] or None, n = nx * ny * nz in C order."""
from __future__ import annotations

import numpy as np

import mesh_oracle as mo
from filter_oracle import fmaf

f32 = np.float32


def empty(shape, color=False, dtype=f32):
    n = int(np.prod(shape))
    return dict(tsdf=np.zeros(n, dtype), weight=np.zeros(n, dtype), color=np.zeros((n, 4), dtype) if color else None)


def centers_f32(shape, affine):
    """[n, 3] float32: p_r = fma(A[r,2], k, fma(A[r,1], j, fma(A[r,0], i, A[r,3])))."""
    A = np.asarray(affine, np.float64).reshape(3, 4).astype(f32)
    i, j, k = (g.reshape(-1).astype(f32) for g in np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"))
    return np.stack([fmaf(A[r, 2], k, fmaf(A[r, 1], j, fmaf(A[r, 0], i, np.full_like(i, A[r, 3])))) for r in range(3)], -1)


def centers_f64(shape, affine):
    A = np.asarray(affine, np.float64).reshape(3, 4)
    idx = np.stack([g.reshape(-1) for g in np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")], -1).astype(np.float64)
    return idx @ A[:, :3].T + A[:, 3]


def _project(p, T, intrinsics, width, height, margin, min_depth, exact):
    """(ok, w, h, z): cr::project."""
    dt = f32 if exact else np.float64
    T = np.asarray(T, dt).reshape(-1)
    fx, fy, cx, cy = (dt(x) for x in intrinsics)
    mul_add = fmaf if exact else (lambda a, b, c: a * b + c)
    q0, q1, q2 = p[:, 0] - T[3], p[:, 1] - T[7], p[:, 2] - T[11]
    c = [mul_add(T[8 + i], q2, mul_add(T[4 + i], q1, T[i] * q0)) for i in range(3)]
    z = c[2]
    ok = z > dt(min_depth)
    u, v = mul_add(fx, c[0] / z, cx), mul_add(fy, c[1] / z, cy)
    w, h = np.rint(u), np.rint(v)                          # half to even
    ok &= (w >= dt(margin)) & (w <= dt(width - 1 - margin)) & (h >= dt(margin)) & (h <= dt(height - 1 - margin))
    return ok, np.where(ok, w, 0).astype(np.int64), np.where(ok, h, 0).astype(np.int64), z


def _integrate(vol, points, depth, t_wc, intrinsics, trunc, max_weight, rgbx, inst, obj_id, slots, margin, min_depth, max_depth, exact):
    dt = f32 if exact else np.float64
    mul_add = fmaf if exact else (lambda a, b, c: a * b + c)
    depth = np.asarray(depth, f32)
    t_wc = np.asarray(t_wc, f32).reshape(-1, 4, 4)
    width, height = depth.shape[1:]
    D, W = vol["tsdf"].astype(dt), vol["weight"].astype(dt)
    C = None if vol["color"] is None else vol["color"].astype(dt)
    p = np.asarray(points, dt)
    tr, mw, one = dt(trunc), dt(max_weight), dt(1)
    for s in (range(len(t_wc)) if slots is None else [int(x) for x in slots]):
        with np.errstate(all="ignore"):
            ok, w, h, z = _project(p, t_wc[s, :3].astype(dt), intrinsics, width, height, margin, min_depth, exact)
            d = depth[s][w, h].astype(dt)
            ok &= (d > dt(min_depth)) & (d <= dt(max_depth))
            if obj_id is not None and obj_id >= 0:
                ok &= np.asarray(inst[s])[w, h] == obj_id
            sdf = d - z
            ok &= sdf >= -tr
            sv = np.fmin(one, sdf / tr)
            W1 = W + one
            D = np.where(ok, mul_add(D, W, sv) / W1, D).astype(dt)
            W = np.where(ok, np.fmin(W1, mw), W).astype(dt)
            if C is not None:
                band = ok & (sdf <= tr)
                wc = C[:, 3].copy()
                wc1 = wc + one
                px = np.asarray(rgbx[s])[w, h].astype(dt)
                for ch in range(3):
                    C[:, ch] = np.where(band, mul_add(C[:, ch], wc, px[:, ch]) / wc1, C[:, ch])
                C[:, 3] = np.where(band, np.fmin(wc1, mw), wc)
    return dict(tsdf=D, weight=W, color=C)


def integrate_f32(vol, shape, affine, depth, t_wc, intrinsics, *, trunc, max_weight=64.0, rgbx=None, inst=None, obj_id=None, slots=None,
                  margin=0, min_depth=0.0, max_depth=np.inf):
    """The exact layer: a new volume dict, every array float32."""
    return _integrate(vol, centers_f32(shape, affine), depth, t_wc, intrinsics, trunc, max_weight, rgbx, inst, obj_id, slots, margin,
                      min_depth, max_depth, True)


def integrate_f64(vol, shape, affine, depth, t_wc, intrinsics, *, trunc, max_weight=64.0, rgbx=None, inst=None, obj_id=None, slots=None,
                  margin=0, min_depth=0.0, max_depth=np.inf):
    """The plain layer: float64 throughout (the inputs are the float32 images and poses)."""
    return _integrate(vol, centers_f64(shape, affine), depth, t_wc, intrinsics, trunc, max_weight, rgbx, inst, obj_id, slots, margin,
                      min_depth, max_depth, False)


# ---- marching cubes over valid points only -------------------------------------------------------------------------------------------
def masked_gradient(vol, valid):
    """[nx, ny, nz, 3] float32: numpy.gradient's stencil with an invalid neighbour treated like the border; 0 with neither side."""
    vol = np.asarray(vol, f32)
    valid = np.asarray(valid) != 0
    out = np.zeros(vol.shape + (3,), f32)
    for ax in range(3):
        v = np.moveaxis(vol, ax, 0)
        m = np.moveaxis(valid, ax, 0)
        pad_v = np.concatenate([v[:1], v, v[-1:]])
        pad_m = np.concatenate([np.zeros_like(m[:1]), m, np.zeros_like(m[:1])])
        lo, hi = pad_m[:-2], pad_m[2:]
        vm, vp = pad_v[:-2], pad_v[2:]
        with np.errstate(all="ignore"):
            g = np.where(lo & hi, (vp - vm) * f32(0.5), np.where(hi, vp - v, np.where(lo, v - vm, f32(0)))).astype(f32)
        out[..., ax] = np.moveaxis(g, 0, ax)
    return out


def marching_cubes(vol, valid, level=0.0, affine=None):
    """-> (vertices [V,3] float32, faces [F,3] int32, normals [V,3] float32, edge_ids [V] int64 = point * 3 + axis, t [V] float32),
    in the kernels' order: vertices by owning point then axis, faces by cell then table order.  A cell exists iff its eight corners are
    valid; an edge's crossing is a vertex iff a cell around the edge exists."""
    vol = np.ascontiguousarray(vol, f32)
    valid = np.ascontiguousarray(np.asarray(valid) != 0)
    nx, ny, nz = vol.shape
    lev = f32(level)
    with np.errstate(invalid="ignore"):
        above = vol > lev
    cell = np.ones((nx - 1, ny - 1, nz - 1), bool)
    for di, dj, dk in mo.CORNERS:
        cell &= valid[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk]
    P = np.zeros((nx + 1, ny + 1, nz + 1), bool)             # P[i + 1, j + 1, k + 1] = cell[i, j, k]; False outside
    P[1:nx, 1:ny, 1:nz] = cell
    cross = np.zeros(vol.shape + (3,), bool)
    cross[:-1, :, :, 0] = above[:-1] != above[1:]
    cross[:, :-1, :, 1] = above[:, :-1] != above[:, 1:]
    cross[:, :, :-1, 2] = above[:, :, :-1] != above[:, :, 1:]
    cross[..., 0] &= P[1:, 1:, 1:] | P[1:, :-1, 1:] | P[1:, 1:, :-1] | P[1:, :-1, :-1]
    cross[..., 1] &= P[1:, 1:, 1:] | P[:-1, 1:, 1:] | P[1:, 1:, :-1] | P[:-1, 1:, :-1]
    cross[..., 2] &= P[1:, 1:, 1:] | P[:-1, 1:, 1:] | P[1:, :-1, 1:] | P[:-1, :-1, 1:]
    flat = cross.reshape(-1)
    edge_ids = np.flatnonzero(flat)
    vid_of_edge = np.full(flat.size, -1, np.int64)
    vid_of_edge[edge_ids] = np.arange(edge_ids.size)
    pt, ax = edge_ids // 3, edge_ids % 3
    idx = np.stack(np.unravel_index(pt, vol.shape), -1).reshape(-1, 3)
    idx1 = idx.copy()
    idx1[np.arange(len(idx1)), ax] += 1
    v0, v1 = vol[tuple(idx.T)], vol[tuple(idx1.T)]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((lev - v0) / (v1 - v0)).astype(f32)
    pos = idx.astype(f32)
    pos[np.arange(len(pos)), ax] += t
    g = masked_gradient(vol, valid)
    tt = t[:, None]
    nrm = -(g[tuple(idx.T)] * (f32(1) - tt) + g[tuple(idx1.T)] * tt)

    cube = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (di, dj, dk) in enumerate(mo.CORNERS):
        cube |= above[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk].astype(np.int64) << c
    cube[~cell] = 0
    cells = np.flatnonzero(mo.TRI_COUNT[cube.reshape(-1)] > 0)
    cidx = np.stack(np.unravel_index(cells, cube.shape), -1) if cells.size else np.zeros((0, 3), np.int64)
    tris = mo.TABLE[cube.reshape(-1)[cells]].astype(np.int64)
    faces = []
    for s in range(5):
        e = tris[:, 3 * s:3 * s + 3]
        ok = e[:, 0] >= 0
        if not ok.any():
            continue
        owner = cidx[ok][:, None, :] + mo.EDGE_OWNER[e[ok]]
        opt = (owner[..., 0] * ny + owner[..., 1]) * nz + owner[..., 2]
        v = vid_of_edge[opt * 3 + mo.EDGE_AXIS[e[ok]]]
        assert (v >= 0).all()
        faces.append((cells[ok] * 8 + s, v))
    if faces:
        key = np.concatenate([k for k, _ in faces])
        f = np.concatenate([v for _, v in faces])[np.argsort(key, kind="stable")].astype(np.int32)
    else:
        f = np.zeros((0, 3), np.int32)
    if affine is not None:
        A = np.asarray(affine, np.float64).reshape(3, 4)
        pos = (pos.astype(np.float64) @ A[:, :3].T + A[:, 3]).astype(f32)
        nrm = (nrm.astype(np.float64) @ np.linalg.inv(A[:, :3])).astype(f32)
    nn = np.sqrt((nrm.astype(np.float64) ** 2).sum(1, keepdims=True))
    nrm = np.where(nn > 0, nrm / np.where(nn > 0, nn, 1), 0).astype(f32)
    return pos, f, nrm, edge_ids, t


def extract(vol, shape, affine, min_weight=1.0):
    """The mesh of a fused volume the way TSDFVolume.extract_mesh defines it: marching cubes of -tsdf at level 0 over the voxels with
    weight >= min_weight (the TSDF is negative inside, so 'above' means inside and the normals, which point to decreasing values,
    point to free space).  -> marching_cubes' tuple."""
    D = -np.asarray(vol["tsdf"], f32).reshape(shape)
    return marching_cubes(D, np.asarray(vol["weight"]).reshape(shape) >= min_weight, 0.0, affine)


def vertex_colors(vol, shape, edge_ids, t):
    """uint8 [V, 3]: the lerp of the edge's two voxel colours at t, rounded half to even."""
    stride = np.array([shape[1] * shape[2], shape[2], 1])
    p0 = edge_ids // 3
    p1 = p0 + stride[edge_ids % 3]
    c0, c1 = np.asarray(vol["color"], f32)[p0, :3], np.asarray(vol["color"], f32)[p1, :3]
    tt = np.asarray(t, f32)[:, None]
    return np.clip(np.rint(c0 + (c1 - c0) * tt), 0, 255).astype(np.uint8)
