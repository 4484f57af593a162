"""TEST INFRASTRUCTURE: the numpy checker of the depth tracker, written from the contract in vmap_amd/csrc/icp_rules.h (not from the
kernels).  Two layers:

- the EXACT layer (``maps``, ``correspond``, ``sums``, ``solve``, ``track``): float32 / float64 in the pinned order, every fused
  multiply-add emulated exactly (filter_oracle.fmaf), the 29 integer sums, the LDL^T solve and the Cayley update in Python floats
  (IEEE float64, one rounding per operation).  The host program and the device must equal it bit for bit.
- the PLAIN layer (``track_plain``): a float64 Gauss-Newton point-to-plane ICP over the same schedule with float64 maps, no
  quantisation, numpy's solver and the exponential map: the geometric yardstick.

Images are [W, H]; a pose is the 12 floats of rows 0 .. 2 of the source-camera -> model-camera matrix."""
from dataclasses import dataclass

import numpy as np

from filter_oracle import fmaf

f32 = np.float32
OK, DEGENERATE, SKIPPED = 0, 1, 2
INLIER, NO_NORMAL, OUTSIDE, NO_MODEL, FAR, ANGLE, GUARD = range(7)
QUANT = 2.0 ** 30
GUARD_LIMIT = 64.0
MAX_PIXELS = 1 << 20


@dataclass
class Params:
    min_depth: float = 0.1
    max_depth: float = 10.0
    band: float = 0.25
    dist_thresh: float = 0.15
    cos_thresh: float = 0.8
    damping: float = 0.0
    pivot_rel: float = 1e-3
    eps: float = 1e-6
    min_inliers: int = 12


def level_sizes(width, height, levels):
    out = []
    for _ in range(levels):
        out.append((width, height))
        width, height = (width + 1) // 2, (height + 1) // 2
    return out


def level_camera(intrinsics, level):
    fx, fy, cx, cy = (f32(v) for v in intrinsics)
    s, off = f32(1 << level), f32((1 << level) - 1) * f32(0.5)
    return fx / s, fy / s, (cx - off) / s, (cy - off) / s


def valid(d, p):
    with np.errstate(invalid="ignore"):
        return (d > f32(p.min_depth)) & (d <= f32(p.max_depth))


def clean(depth, p):
    d = np.asarray(depth, f32)
    return np.where(valid(d, p), d, f32(0))


def down(D, p):
    W, H = D.shape
    W2, H2 = (W + 1) // 2, (H + 1) // 2
    wa, ha = 2 * np.arange(W2), 2 * np.arange(H2)
    wb, hb = np.minimum(wa + 1, W - 1), np.minimum(ha + 1, H - 1)
    s = np.zeros((W2, H2), f32)
    mn, mx = s.copy(), s.copy()
    n = np.zeros((W2, H2), np.int32)
    for ws, hs in ((wa, ha), (wb, ha), (wa, hb), (wb, hb)):
        v = D[np.ix_(ws, hs)]
        ok = valid(v, p)
        first = ok & (n == 0)
        later = ok & (n > 0)
        s = np.where(first, v, np.where(later, s + v, s)).astype(f32)
        mn = np.where(first, v, np.where(later & (v < mn), v, mn))
        mx = np.where(first, v, np.where(later & (v > mx), v, mx))
        n = n + ok
    keep = (n > 0) & ((mx - mn).astype(f32) <= f32(p.band))
    return np.where(keep, s / np.maximum(n, 1).astype(f32), f32(0)).astype(f32)


def vertex(cam, w, h, d):
    fx, fy, cx, cy = cam
    return [(np.asarray(w).astype(f32) - cx) / fx * d, (np.asarray(h).astype(f32) - cy) / fy * d, d]


def level_map(D, cam, p):
    """[W, H, 4] float32: (n0, n1, n2, d) per pixel of a cleaned level."""
    W, H = D.shape
    out = np.zeros((W, H, 4), f32)
    out[..., 3] = D
    if W < 3 or H < 3:
        return out
    w, h = np.meshgrid(np.arange(1, W - 1), np.arange(1, H - 1), indexing="ij")
    d, dwm, dwp, dhm, dhp = D[1:-1, 1:-1], D[:-2, 1:-1], D[2:, 1:-1], D[1:-1, :-2], D[1:-1, 2:]
    with np.errstate(all="ignore"):
        ok = valid(d, p) & valid(dwm, p) & valid(dwp, p) & valid(dhm, p) & valid(dhp, p)
        two = f32(p.band) + f32(p.band)
        ok &= (np.abs(dwp - dwm) <= two) & (np.abs(dhp - dhm) <= two)
        P, Wp, Wm = vertex(cam, w, h, d), vertex(cam, w + 1, h, dwp), vertex(cam, w - 1, h, dwm)
        Hp, Hm = vertex(cam, w, h + 1, dhp), vertex(cam, w, h - 1, dhm)
        a = [Wp[k] - Wm[k] for k in range(3)]
        b = [Hp[k] - Hm[k] for k in range(3)]
        c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        length = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
        ok &= length > 0
        n = [c[k] / length for k in range(3)]
        flip = n[0] * P[0] + n[1] * P[1] + n[2] * P[2] > 0
        for k in range(3):
            out[1:-1, 1:-1, k] = np.where(ok, np.where(flip, -n[k], n[k]), f32(0))
    return out


def maps(depth, intrinsics, levels, p):
    """The exact maps of a depth image [W, H]: a list, level 0 first, of [W_l, H_l, 4] float32."""
    D = clean(depth, p)
    out = []
    for level in range(levels):
        if level:
            D = down(D, p)
        out.append(level_map(D, level_camera(intrinsics, level), p))
    return out


def pose_rows(T64):
    return np.asarray(T64, np.float64).reshape(12).astype(f32)


def correspond(src, model, cam, T64, p):
    """Every source pixel's fate under the pose: (reason [W, H], r [W, H] float64, J [W, H, 6] float64; r and J hold numbers where
    reason is INLIER or GUARD)."""
    W, H = src.shape[:2]
    T = pose_rows(T64)
    fx, fy, cx, cy = cam
    w, h = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    reason = np.full((W, H), INLIER, np.int32)
    with np.errstate(all="ignore"):
        has = (src[..., 0] != 0) | (src[..., 1] != 0) | (src[..., 2] != 0)
        reason[~has] = NO_NORMAL
        pt = vertex(cam, w, h, src[..., 3])
        pp = [(fmaf(T[4 * i + 2], pt[2], fmaf(T[4 * i + 1], pt[1], T[4 * i] * pt[0])) + T[4 * i + 3]).astype(f32) for i in range(3)]
        npr = [fmaf(T[4 * i + 2], src[..., 2], fmaf(T[4 * i + 1], src[..., 1], T[4 * i] * src[..., 0])) for i in range(3)]
        z = pp[2]
        front = z > f32(p.min_depth)
        wf, hf = np.rint(fmaf(fx, pp[0] / z, cx)), np.rint(fmaf(fy, pp[1] / z, cy))
        inside = front & (wf >= 0) & (wf <= f32(W - 1)) & (hf >= 0) & (hf <= f32(H - 1))
        reason[(reason == INLIER) & ~inside] = OUTSIDE
        wm = np.where(inside, wf, 0).astype(np.int64)
        hm = np.where(inside, hf, 0).astype(np.int64)
        m = model[wm, hm]
        live = reason == INLIER
        reason[live & ~((m[..., 0] != 0) | (m[..., 1] != 0) | (m[..., 2] != 0))] = NO_MODEL
        live = reason == INLIER
        reason[live & ~(np.abs(z - m[..., 3]) <= f32(p.dist_thresh))] = FAR
        live = reason == INLIER
        dot = npr[0] * m[..., 0] + npr[1] * m[..., 1] + npr[2] * m[..., 2]
        reason[live & ~(dot >= f32(p.cos_thresh))] = ANGLE
        q = vertex(cam, wm, hm, m[..., 3])
        P = [x.astype(np.float64) for x in pp]
        M = [m[..., k].astype(np.float64) for k in range(3)]
        e = [P[k] - q[k].astype(np.float64) for k in range(3)]
        r = M[0] * e[0] + M[1] * e[1] + M[2] * e[2]
        J = np.stack([M[0], M[1], M[2], P[1] * M[2] - P[2] * M[1], P[2] * M[0] - P[0] * M[2], P[0] * M[1] - P[1] * M[0]], -1)
        guard = (np.abs(r) <= GUARD_LIMIT) & (np.abs(J) <= GUARD_LIMIT).all(-1)
        reason[(reason == INLIER) & ~guard] = GUARD
    return reason, r, J


def quant(x):
    return np.rint(np.asarray(x, np.float64) * QUANT).astype(np.int64)


def pair_sums(r, J):
    """The 29 integers of pairs (r [N], J [N, 6]), summed."""
    r, J = np.asarray(r, np.float64).reshape(-1), np.asarray(J, np.float64).reshape(-1, 6)
    out = [np.int64(len(r))]
    for i in range(6):
        for j in range(i, 6):
            out.append(quant(J[:, i] * J[:, j]).sum(dtype=np.int64))
    for k in range(6):
        out.append(quant(J[:, k] * r).sum(dtype=np.int64))
    out.append(quant(r * r).sum(dtype=np.int64))
    return np.array(out, np.int64)


def sums(src, model, cam, T64, p):
    reason, r, J = correspond(src, model, cam, T64, p)
    keep = reason == INLIER
    return pair_sums(r[keep], J[keep])


def solve(s, T64, p):
    """Section 5 in Python floats.  -> (status, finished, x [6], |x|^2, the new pose [12])."""
    T = [float(v) for v in np.asarray(T64, np.float64).reshape(12)]
    zero = [0.0] * 6
    s = [int(v) for v in s]
    if s[0] < int(p.min_inliers):
        return DEGENERATE, 0, zero, 0.0, T
    inv = 1.0 / QUANT
    A = [[0.0] * 6 for _ in range(6)]
    at = 1
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(s[at]) * inv
            at += 1
    b = [0.0] * 6
    for k in range(6):
        A[k][k] = A[k][k] + float(p.damping)
        b[k] = float(s[22 + k]) * inv
    top = A[0][0]
    for k in range(1, 6):
        top = A[k][k] if A[k][k] > top else top
    thresh = float(p.pivot_rel) * top
    L = [[0.0] * 6 for _ in range(6)]
    D, w = [0.0] * 6, [0.0] * 6
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            w[k] = L[j][k] * D[k]
            d = d - L[j][k] * w[k]
        if not d > thresh:
            return DEGENERATE, 0, zero, 0.0, T
        D[j] = d
        for i in range(j + 1, 6):
            acc = A[i][j]
            for k in range(j):
                acc = acc - L[i][k] * w[k]
            L[i][j] = acc / d
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        acc = -b[i]
        for k in range(i):
            acc = acc - L[i][k] * y[k]
        y[i] = acc
    for i in range(5, -1, -1):
        acc = y[i] / D[i]
        for k in range(i + 1, 6):
            acc = acc - L[k][i] * x[k]
        x[i] = acc
    x2 = x[0] * x[0]
    for k in range(1, 6):
        x2 = x2 + x[k] * x[k]
    if not np.isfinite(x2):
        return DEGENERATE, 0, zero, 0.0, T
    R = cayley(x[3:])
    N = [0.0] * 12
    for i in range(3):
        for j in range(3):
            N[4 * i + j] = R[i][0] * T[j] + R[i][1] * T[4 + j] + R[i][2] * T[8 + j]
        N[4 * i + 3] = R[i][0] * T[3] + R[i][1] * T[7] + R[i][2] * T[11] + x[i]
    eps = float(p.eps)
    return OK, int(x2 < eps * eps), x, x2, N


def cayley(omega):
    a0, a1, a2 = (0.5 * float(v) for v in omega)
    ss = a0 * a0 + a1 * a1 + a2 * a2
    den, c = 1.0 + ss, 1.0 - ss
    return [[(c + 2.0 * (a0 * a0)) / den, (2.0 * (a0 * a1) + 2.0 * -a2) / den, (2.0 * (a0 * a2) + 2.0 * a1) / den],
            [(2.0 * (a1 * a0) + 2.0 * a2) / den, (c + 2.0 * (a1 * a1)) / den, (2.0 * (a1 * a2) + 2.0 * -a0) / den],
            [(2.0 * (a2 * a0) + 2.0 * -a1) / den, (2.0 * (a2 * a1) + 2.0 * a0) / den, (c + 2.0 * (a2 * a2)) / den]]


def track_maps(src_maps, model_maps, T0, intrinsics, iterations, p):
    """The chain of a track call on given maps.  iterations[l] belongs to level l; levels run coarse first.  -> dict: log [n, 4],
    sums [n, 29], poses [n, 12] (after every iteration), pose [12]."""
    T = [float(v) for v in np.asarray(T0, np.float64).reshape(12)]
    log, all_sums, poses = [], [], []
    for level in range(len(iterations) - 1, -1, -1):
        cam = level_camera(intrinsics, level)
        done = False
        for _ in range(iterations[level]):
            if done:
                log.append([0.0, 0.0, float(SKIPPED), 0.0])
                all_sums.append(np.zeros(29, np.int64))
            else:
                s = sums(src_maps[level], model_maps[level], cam, T, p)
                status, finished, _, x2, T = solve(s, T, p)
                log.append([float(int(s[0])), float(int(s[28])) * (1.0 / QUANT), float(status), x2])
                all_sums.append(s)
                done = bool(finished)
            poses.append(list(T))
    return dict(log=np.array(log, np.float64).reshape(-1, 4), sums=np.array(all_sums, np.int64).reshape(-1, 29),
                poses=np.array(poses, np.float64).reshape(-1, 12), pose=np.array(T, np.float64))


def track(depth, model_depth, T0, intrinsics, iterations, p):
    levels = len(iterations)
    out = track_maps(maps(depth, intrinsics, levels, p), maps(model_depth, intrinsics, levels, p), T0, intrinsics, iterations, p)
    return out


def summary(out, n_level0, pixels):
    """ok and inlier_fraction of a track result as vmap_amd.odometry defines them: the last row of level 0 that is not SKIPPED."""
    rows = out["log"][-n_level0:]
    live = [r for r in rows if int(r[2]) != SKIPPED]
    return int(live[-1][2]) == OK, float(live[-1][0]) / pixels


# ---- the plain float64 layer ---------------------------------------------------------------------------------------------------------
def _maps64(depth, intrinsics, levels, p):
    D = np.asarray(depth, np.float64)
    with np.errstate(invalid="ignore"):
        D = np.where((D > p.min_depth) & (D <= p.max_depth), D, 0.0)
    out = []
    for level in range(levels):
        if level:
            W, H = D.shape
            wa, ha = 2 * np.arange((W + 1) // 2), 2 * np.arange((H + 1) // 2)
            wb, hb = np.minimum(wa + 1, W - 1), np.minimum(ha + 1, H - 1)
            v = np.stack([D[np.ix_(a, b)] for a, b in ((wa, ha), (wb, ha), (wa, hb), (wb, hb))])
            ok = v > 0
            n = ok.sum(0)
            big = np.where(ok, v, -np.inf).max(0)
            small = np.where(ok, v, np.inf).min(0)
            with np.errstate(all="ignore"):
                D = np.where((n > 0) & (big - small <= p.band), np.where(ok, v, 0).sum(0) / np.maximum(n, 1), 0.0)
        s = float(1 << level)
        fx, fy = intrinsics[0] / s, intrinsics[1] / s
        cx, cy = (intrinsics[2] - ((1 << level) - 1) / 2) / s, (intrinsics[3] - ((1 << level) - 1) / 2) / s
        W, H = D.shape
        w, h = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="ij")
        V = np.stack([(w - cx) / fx * D, (h - cy) / fy * D, D], -1)
        N = np.zeros((W, H, 3))
        if W >= 3 and H >= 3:
            ok = (D[1:-1, 1:-1] > 0) & (D[:-2, 1:-1] > 0) & (D[2:, 1:-1] > 0) & (D[1:-1, :-2] > 0) & (D[1:-1, 2:] > 0)
            ok &= (np.abs(D[2:, 1:-1] - D[:-2, 1:-1]) <= 2 * p.band) & (np.abs(D[1:-1, 2:] - D[1:-1, :-2]) <= 2 * p.band)
            c = np.cross(V[2:, 1:-1] - V[:-2, 1:-1], V[1:-1, 2:] - V[1:-1, :-2])
            length = np.linalg.norm(c, axis=-1)
            ok &= length > 0
            with np.errstate(all="ignore"):
                n = c / length[..., None]
            n = np.where(((n * V[1:-1, 1:-1]).sum(-1) > 0)[..., None], -n, n)
            N[1:-1, 1:-1] = np.where(ok[..., None], n, 0.0)
        out.append((D, V, N, (fx, fy, cx, cy)))
    return out


def rodrigues(omega):
    omega = np.asarray(omega, np.float64)
    th = float(np.linalg.norm(omega))
    K = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def track_plain(depth, model_depth, T0, intrinsics, iterations, p):
    """Float64 Gauss-Newton point-to-plane ICP over the same schedule: numpy's solver, the exponential map, no quantisation, no early
    finish.  -> the pose [12]."""
    levels = len(iterations)
    src, mod = _maps64(depth, intrinsics, levels, p), _maps64(model_depth, intrinsics, levels, p)
    T = np.eye(4)
    T[:3] = np.asarray(T0, np.float64).reshape(3, 4)
    for level in range(levels - 1, -1, -1):
        Ds, Vs, Ns, (fx, fy, cx, cy) = src[level]
        Dm, Vm, Nm, _ = mod[level]
        W, H = Ds.shape
        has = (Ns != 0).any(-1)
        for _ in range(iterations[level]):
            P = Vs[has] @ T[:3, :3].T + T[:3, 3]
            Nr = Ns[has] @ T[:3, :3].T
            with np.errstate(all="ignore"):
                wf, hf = np.rint(fx * P[:, 0] / P[:, 2] + cx), np.rint(fy * P[:, 1] / P[:, 2] + cy)
                ok = (P[:, 2] > p.min_depth) & (wf >= 0) & (wf <= W - 1) & (hf >= 0) & (hf <= H - 1)
            wm, hm = np.where(ok, wf, 0).astype(int), np.where(ok, hf, 0).astype(int)
            M, Q = Nm[wm, hm], Vm[wm, hm]
            ok &= (M != 0).any(-1) & (np.abs(P[:, 2] - Dm[wm, hm]) <= p.dist_thresh) & ((Nr * M).sum(-1) >= p.cos_thresh)
            P, M, Q = P[ok], M[ok], Q[ok]
            if len(P) < 6:
                break
            r = (M * (P - Q)).sum(-1)
            J = np.concatenate([M, np.cross(P, M)], -1)
            x = np.linalg.solve(J.T @ J + p.damping * np.eye(6), -(J.T @ r))
            dT = np.eye(4)
            dT[:3, :3], dT[:3, 3] = rodrigues(x[3:]), x[:3]
            T = dT @ T
    return T[:3].reshape(12)


def pose_error(T, T_true):
    """The Frobenius distance of two poses' rows 0 .. 2 (rotation entries and metres together)."""
    return float(np.linalg.norm(np.asarray(T, np.float64).reshape(12) - np.asarray(T_true, np.float64).reshape(12)))
