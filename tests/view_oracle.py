"""Checker of the view renderer (vmap_amd/render.py, csrc/view_kernels.h, csrc/view_geometry.h): the contract of the view section of
include/vmapstep.h in float64 numpy, a float32 emulation of its geometry that is exact operation by operation (fused multiply-adds
included), the standard scene of the tests and the build of the host program tests/tools/view_geometry_host.cpp.
Independent of the package: nothing here imports vmap_amd."""
import math
import os
import subprocess

import numpy as np

import bounds_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_HITS = 16
EDGE = 1e-4                                 # pixels where a float64 |t_far - t_near| of any object is below this are "edge pixels"
f32, f64 = np.float32, np.float64


class Box:
    def __init__(self, center, R, extent):
        self.center, self.R, self.extent = np.asarray(center, f64), np.asarray(R, f64), np.asarray(extent, f64)

    def row(self):
        return np.concatenate([self.center, self.R.reshape(-1), self.extent]).astype(f32)


def ring_pose(az, el, radius=3.0):
    """bounds_oracle.Scene's camera: on a sphere of ``radius`` around the origin, looking at it, x horizontal."""
    pos = radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    z = -pos / np.linalg.norm(pos)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, pos
    return T.astype(f32)


class Standard:
    """The standard scene: 96 x 64, fx = 90, principal point in the middle, ring poses at radius 3, min_depth 0.05, four boxes."""
    W, H, FX, MIN_DEPTH, S = 96, 64, 90.0, 0.05, 16
    VIEWS = ((0.3, 0.5), (2.0, -0.6), (4.1, 0.2))

    @staticmethod
    def k4(W=96, H=64, fx=90.0):
        return (fx, fx, (W - 1) / 2.0, (H - 1) / 2.0)

    @staticmethod
    def boxes():
        return [Box((-0.75, 0.05, 0.0), bo.rotation((1, 2, 3), 0.6), (0.6, 0.9, 1.5)),
                Box((0.85, -0.05, 0.05), bo.rotation((-2, 1, 1), 1.1), (1.0, 1.0, 1.0)),
                Box((-0.45, 0.25, 0.2), bo.rotation((0, 1, 1), 0.3), (0.8, 0.5, 0.7)),          # overlaps the first
                Box((0.1, 0.0, -0.9), np.eye(3), (3.0, 3.0, 0.2))]                               # floor slab


# ---- float32 emulation, exact per operation ---------------------------------------------------------------------------------------

def fma32(a, b, c):
    """round32(a * b + c) with ONE rounding, for float32 arrays: the product is exact in float64; the sum is rounded to odd in float64
    (TwoSum gives the error of the rounded sum), and rounding a round-to-odd 53-bit value to 24 bits equals rounding the exact value."""
    p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
    c = np.asarray(c, f32).astype(f64)
    p, c = np.broadcast_arrays(p, c)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def rays32(T, k4, W, H):
    """o [3], d [W * H, 3] in float32 by the contract's operations."""
    fx, fy, cx, cy = (f32(v) for v in k4)
    T = np.asarray(T, f32)
    w, h = np.meshgrid(np.arange(W).astype(f32), np.arange(H).astype(f32), indexing="ij")
    x = ((w - cx) / fx).reshape(-1)
    y = ((h - cy) / fy).reshape(-1)
    d = np.stack([fma32(T[i, 0], x, fma32(T[i, 1], y, np.full_like(x, T[i, 2]))) for i in range(3)], 1)
    return T[:3, 3].copy(), d


def geometry32(T, k4, W, H, boxes, S, min_depth):
    """hit bool [n, P], t_near, dt float32 [n, P]: what view_geometry.h computes, bit for bit."""
    o, d = rays32(T, k4, W, H)
    hits, tns, dts = [], [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in boxes:
            row = b.row()
            c, R, e = row[0:3], row[3:12].reshape(3, 3), row[12:15]
            q = o - c
            near = np.full(len(d), -np.inf, f32)
            far = np.full(len(d), np.inf, f32)
            for i in range(3):
                ob = fma32(R[2, i], q[2], fma32(R[1, i], q[1], R[0, i] * q[0]))
                db = fma32(R[2, i], d[:, 2], fma32(R[1, i], d[:, 1], R[0, i] * d[:, 0]))
                h = f32(0.5) * e[i]
                ta, tb = (-h - ob) / db, (h - ob) / db
                near = np.fmax(near, np.fmin(ta, tb))
                far = np.fmin(far, np.fmax(ta, tb))
            tn = np.fmax(f32(min_depth), near) + f32(0.0)
            hits.append(far > tn)
            tns.append(tn.astype(f32))
            dts.append(((far - tn) / f32(S)).astype(f32))
    return np.stack(hits), np.stack(tns), np.stack(dts)


def sample_depths32(t_near, dt, S):
    """t_s = fma(s + 0.5, dt, t_near): float32 [..., S]."""
    s = (np.arange(S).astype(f32) + f32(0.5))
    return fma32(s, np.asarray(dt, f32)[..., None], np.asarray(t_near, f32)[..., None])


def points32(o, d, t, center):
    """(o + d * t) - center with every operation rounded: o [3], d [m, 3], t [m, S], center [3] -> [m, S, 3] float32."""
    o, d, t, c = np.asarray(o, f32), np.asarray(d, f32), np.asarray(t, f32), np.asarray(center, f32)
    return ((o[None, None, :] + d[:, None, :] * t[:, :, None]) - c[None, None, :]).astype(f32)


# ---- float64 geometry ---------------------------------------------------------------------------------------------------------------

def geometry64(T, k4, W, H, boxes, S, min_depth):
    """The same formulas in float64 on the float32 inputs: hit [n, P], t_near, t_far, dt [n, P], rays (o, d)."""
    fx, fy, cx, cy = (f64(f32(v)) for v in k4)
    T = np.asarray(T, f32).astype(f64)
    w, h = np.meshgrid(np.arange(W, dtype=f64), np.arange(H, dtype=f64), indexing="ij")
    dc = np.stack([((w - cx) / fx).reshape(-1), ((h - cy) / fy).reshape(-1), np.ones(W * H)], 1)
    d = dc @ T[:3, :3].T
    o = T[:3, 3]
    hits, tns, tfs = [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in boxes:
            row = b.row().astype(f64)
            c, R, e = row[0:3], row[3:12].reshape(3, 3), row[12:15]
            ob, db = (o - c) @ R, d @ R
            ta, tb = (-0.5 * e - ob) / db, (0.5 * e - ob) / db
            near = np.fmax.reduce(np.fmin(ta, tb), axis=1, initial=-np.inf)
            far = np.fmin.reduce(np.fmax(ta, tb), axis=1, initial=np.inf)
            tn = np.fmax(f64(f32(min_depth)), near)
            hits.append(far > tn)
            tns.append(tn)
            tfs.append(far)
    hit, tn, tf = np.stack(hits), np.stack(tns), np.stack(tfs)
    return hit, tn, tf, (tf - tn) / S, (o, d)


def geometry_bound(T, k4, W, H, boxes, S, min_depth):
    """A bound on |float32 - float64| of t_near and dt [n, P] each, from the operation order of view_geometry.h (u = 2^-24):
      x = (w - cx) / fx: two roundings; d_i = fma(T_i0, x, fma(T_i1, y, T_i2)): two more and the 2u of x, y carried through:
          eps_d_i <= 4u M_i,  M_i = |T_i0 x| + |T_i1 y| + |T_i2|
      q = o - c: eps_q_j <= u |q_j|;  ob_i = fma(R_2i, q_z, fma(R_1i, q_y, R_0i q_x)): three roundings + eps_q carried:
          eps_ob_i <= 4u A_i,  A_i = sum_j |R_ji q_j|
      db_i likewise from d:  eps_db_i <= 3u sum_j |R_ji d_j| + sum_j |R_ji| eps_d_j
      num = (+-h_i - ob_i) (h_i = 0.5 e_i exact): u |num| + eps_ob;  t = num / db: u |t| and the division amplifies:
          eps_t <= (eps_ob + |t| eps_db) / |db| + 2u |t|
      fmin / fmax are exact and 1-Lipschitz in the maximum norm: eps_near, eps_far <= the largest eps_t over the axes and both
      planes with a finite t;  t_near = fmax(min_depth, near): the same;  dt = (far - t_near) / S: one rounding each:
          eps_dt <= (eps_far + eps_near + u |far - t_near|) / S + u |dt|."""
    u = 2.0 ** -24
    fx, fy, cx, cy = (f64(f32(v)) for v in k4)
    T = np.asarray(T, f32).astype(f64)
    w, h = np.meshgrid(np.arange(W, dtype=f64), np.arange(H, dtype=f64), indexing="ij")
    dc = np.stack([((w - cx) / fx).reshape(-1), ((h - cy) / fy).reshape(-1), np.ones(W * H)], 1)
    d = dc @ T[:3, :3].T
    eps_d = 4 * u * (np.abs(dc) @ np.abs(T[:3, :3]).T)
    o = T[:3, 3]
    b_tn, b_dt = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in boxes:
            row = b.row().astype(f64)
            c, R, e = row[0:3], row[3:12].reshape(3, 3), row[12:15]
            q = o - c
            ob, db = q @ R, d @ R
            eps_ob = 4 * u * (np.abs(q) @ np.abs(R))
            eps_db = 3 * u * (np.abs(d) @ np.abs(R)) + eps_d @ np.abs(R)
            worst = np.zeros(len(d))
            for sign in (-0.5, 0.5):
                t = (sign * e - ob) / db
                eps_t = (eps_ob + np.abs(t) * eps_db) / np.abs(db) + 2 * u * np.abs(t)
                worst = np.maximum(worst, np.where(np.isfinite(t), eps_t, 0.0).max(1))
            ta, tb = (-0.5 * e - ob) / db, (0.5 * e - ob) / db
            near = np.fmax(f64(f32(min_depth)), np.fmax.reduce(np.fmin(ta, tb), axis=1, initial=-np.inf))
            far = np.fmin.reduce(np.fmax(ta, tb), axis=1, initial=np.inf)
            b_tn.append(worst)
            b_dt.append((2 * worst + u * np.abs(far - near)) / S + u * np.abs(far - near) / S)
    return np.stack(b_tn), np.stack(b_dt)


def edge_pixels(tn64, tf64):
    """Pixels where any object's float64 |t_far - t_near| < EDGE (a hit decision there may flip in float32)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(tf64 - tn64) < EDGE).any(0)


# ---- compositing --------------------------------------------------------------------------------------------------------------------

def termination(occ):
    """render_rays.py:26-34 in float64 along the last axis: w_i = occ_i * prod_{j<i} ((1 - occ_j) + 1e-10)."""
    occ = np.asarray(occ, f64)
    free = (1.0 - occ) + 1e-10
    T = np.concatenate([np.ones(occ.shape[:-1] + (1,)), np.cumprod(free[..., :-1], -1)], -1)
    return occ * T


def composite(n_pix, hit, t, occ, rgb, t_near=None, with_sensitivity=False):
    """The contract's merge in float64.  hit bool [n, P]; t [n, P, S] sample depths (used as given: pass the float32 values to order
    exactly as the device does); occ [n, P, S]; rgb [n, P, S, 3].  ``t_near`` [n, P]: applies the MAX_HITS cap by (t_near, k).
    Returns depth, color, opacity, instance, overflow count, per-object weights [P, n] and - with_sensitivity - per output the first-
    order sensitivity  sum_i |d out / d occ_i| + sum_i w_i  (depth, color [P, 3], opacity)."""
    n, P, S = t.shape
    assert P == n_pix
    hit = np.array(hit, bool)
    overflow = 0
    if t_near is not None:
        cnt = hit.sum(0)
        for p in np.nonzero(cnt > MAX_HITS)[0]:
            ks = np.nonzero(hit[:, p])[0]
            order = sorted(ks, key=lambda k: (float(t_near[k, p]), int(k)))
            hit[order[MAX_HITS:], p] = False
            overflow += 1
    tt = np.where(hit[:, :, None], np.asarray(t, f64), np.inf).transpose(1, 0, 2).reshape(P, n * S)
    oc = (np.asarray(occ, f64) * hit[:, :, None]).transpose(1, 0, 2).reshape(P, n * S)
    co = np.asarray(rgb, f64).transpose(1, 0, 2, 3).reshape(P, n * S, 3)
    ob = np.broadcast_to(np.arange(n)[None, :, None], (P, n, S)).reshape(P, n * S)
    order = np.argsort(tt, 1, kind="stable")                 # ties: object-major concatenation = ascending (k, s)
    tt, oc, ob = (np.take_along_axis(a, order, 1) for a in (tt, oc, ob))
    co = np.take_along_axis(co, order[..., None], 1)
    valid = np.isfinite(tt)
    tt = np.where(valid, tt, 0.0)
    w = termination(oc)
    depth, color, opacity = (w * tt).sum(1), (w[..., None] * co).sum(1), w.sum(1)
    wk = np.stack([(w * (ob == k)).sum(1) for k in range(n)], 1)
    wk_hit = np.where(hit.T, wk, -1.0)
    instance = np.where(hit.any(0), wk_hit.argmax(1), -1).astype(np.int32)
    out = dict(depth=depth, color=color, opacity=opacity, instance=instance, overflow=overflow, weights=wk, n_hits=hit.sum(0))
    if with_sensitivity:
        free = (1.0 - oc) + 1e-10
        N = n * S
        sens = {"depth": np.zeros(P), "color": np.zeros((P, 3)), "opacity": np.zeros(P)}
        vals = {"depth": tt[..., None], "color": co, "opacity": np.ones((P, N, 1))}
        for i in range(N):
            # d w_j / d occ_i: the transmittance in front of i for j = i; -occ_j * prod_{m<j, m != i} free_m for j > i
            fr = free.copy()
            fr[:, i] = 1.0
            Tx = np.concatenate([np.ones((P, 1)), np.cumprod(fr[:, :-1], 1)], 1)
            dw = np.zeros((P, N))
            dw[:, i] = Tx[:, i]
            dw[:, i + 1:] = -oc[:, i + 1:] * Tx[:, i + 1:]
            for key, v in vals.items():
                g = np.abs((dw[..., None] * v).sum(1)) * valid[:, i, None]
                sens[key] += g[:, 0] if key != "color" else g
        for key in sens:
            sens[key] = sens[key] + (opacity if key != "color" else opacity[:, None])
        out["sensitivity"] = sens
    return out


# ---- the host program ---------------------------------------------------------------------------------------------------------------

def build_host_program(out_dir, extra_flags=()):
    """g++ -O2 -ffp-contract=off of tests/tools/view_geometry_host.cpp against csrc/view_geometry.h -> the executable's path."""
    exe = os.path.join(str(out_dir), "view_geometry_host" + ("_san" if extra_flags else ""))
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", *extra_flags, "-I", os.path.join(ROOT, "vmap_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "view_geometry_host.cpp"), "-o", exe], check=True)
    return exe


def run_host_program(exe, out_dir, T, k4, W, H, boxes, S, min_depth):
    """hit bool [n, P], t_near, dt float32 [n, P] as the host program prints them (inputs handed over as hexadecimal floats)."""
    hx = lambda v: float(f32(v)).hex()
    path = os.path.join(str(out_dir), "view_scene.txt")
    with open(path, "w") as fh:
        fh.write(f"{W} {H} {S} {len(boxes)}\n" + " ".join(hx(v) for v in (*k4, min_depth)) + "\n")
        fh.write(" ".join(hx(v) for v in np.asarray(T, f32).reshape(-1)) + "\n")
        for b in boxes:
            fh.write(" ".join(hx(v) for v in b.row()) + "\n")
    tok = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split()
    n, P = len(boxes), W * H
    assert len(tok) == 3 * n * P, (len(tok), n, P)
    hit = np.array(tok[0::3], np.int64).astype(bool).reshape(n, P)
    tn = np.array([int(x, 16) for x in tok[1::3]], np.uint32).view(f32).reshape(n, P)
    dt = np.array([int(x, 16) for x in tok[2::3]], np.uint32).view(f32).reshape(n, P)
    return hit, tn, dt


def pairs_of(hit, t_near, dt, pix_begin=0, pix_end=None):
    """The pair list view_emit must write for a pixel range: (offsets int64 [n + 1], pixel int32 [m], t_near [m], dt [m]) ordered by
    (object, pixel)."""
    n, P = hit.shape
    pix_end = P if pix_end is None else pix_end
    offs, px, tn, d = [0], [], [], []
    for k in range(n):
        idx = np.nonzero(hit[k, pix_begin:pix_end])[0] + pix_begin
        px.append(idx.astype(np.int32)); tn.append(t_near[k, idx]); d.append(dt[k, idx])
        offs.append(offs[-1] + len(idx))
    return np.asarray(offs, np.int64), np.concatenate(px), np.concatenate(tn).astype(f32), np.concatenate(d).astype(f32)


# ---- the whole renderer in float64 --------------------------------------------------------------------------------------------------

def field64(fc, B, scale, k, pts):
    """Occupancy [m] and colour [m, 3] of object k at the points [m, 3], by oracle/vmap_oracle.py in float64."""
    from oracle import vmap_oracle as ref
    emb = ref.positional_encoding(np.asarray(pts, f64)[None, :, None, :], np.asarray(B[k], f64)[None], np.asarray([scale[k]], f64), dtype=f64)[0]
    alpha, color = ref.field_forward(emb, [np.asarray(a, f64)[k][None] for a in fc], dtype=f64)[:2]
    return 1.0 / (1.0 + np.exp(-alpha.reshape(-1))), color.reshape(-1, 3)


def render_checker(T, k4, W, H, boxes, centers, S, min_depth, params, geometry="float64", with_sensitivity=False):
    """The contract end to end: geometry in float64 ("float64") or by the float32 emulation ("float32": hits, t_s and points rounded as
    the device rounds them), the field and the composite in float64.  Returns composite()'s dict + hit, and the float64 edge pixels."""
    fc, B, scale = params
    n, P = len(boxes), W * H
    hit64, tn64, tf64, dt64, (o64, d64) = geometry64(T, k4, W, H, boxes, S, min_depth)
    if geometry == "float32":
        hit, tn, dt = geometry32(T, k4, W, H, boxes, S, min_depth)
        o, d = rays32(T, k4, W, H)
    else:
        hit, tn, dt, o, d = hit64, tn64, dt64, o64, d64
    t = np.zeros((n, P, S))
    occ = np.zeros((n, P, S))
    rgb = np.zeros((n, P, S, 3))
    for k in range(n):
        idx = np.nonzero(hit[k])[0]
        if not len(idx):
            continue
        if geometry == "float32":
            ts = sample_depths32(tn[k, idx], dt[k, idx], S)
            pts = points32(o, d[idx], ts, centers[k])
        else:
            ts = tn[k, idx, None] + (np.arange(S) + 0.5)[None] * dt[k, idx, None]
            pts = (o[None, None] + d[idx, None, :] * ts[..., None]) - np.asarray(f32(centers[k]), f64)[None, None]
        oc, co = field64(fc, B, scale, k, pts.reshape(-1, 3))
        t[k, idx], occ[k, idx], rgb[k, idx] = ts, oc.reshape(-1, S), co.reshape(-1, S, 3)
    out = composite(P, hit, t, occ, rgb, t_near=np.where(hit, tn, np.inf), with_sensitivity=with_sensitivity)
    out["hit"], out["edge"] = hit, edge_pixels(tn64, tf64)
    return out
