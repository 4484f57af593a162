"""Float64 numpy checker for the object bounds (vmap_amd/bounds.py, csrc/bounds_kernels.h): unprojection of keyframes, extents of a
cloud along given frames, an exhaustive fixed-grid box search for small clouds, analytic test clouds and a synthetic scene of boxes
seen by pinhole cameras on a ring.  Independent of the package: nothing here imports vmap_amd."""
import math

import numpy as np


# ---- rotations ---------------------------------------------------------------------------------------------------------------------

def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


# ---- unprojection ------------------------------------------------------------------------------------------------------------------

def unproject(depth, inst, t_wc, k4, obj_id):
    """The world points of one frame (depth [W, H], inst [W, H], t_wc [4, 4], all as stored: float32 / int32) for ``obj_id``, in
    pixel-index order w * H + h, computed in float64; also per point and coordinate the magnitude sum |T_i0 x| + |T_i1 y| + |T_i2 d|
    + |t_i| that a rounding bound of the float32 evaluation scales with."""
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in k4)
    W, H = depth.shape
    w, h = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    keep = (inst == obj_id) & (depth > 0)
    d = depth[keep].astype(np.float64)
    x = (w[keep] - cx) / fx * d
    y = (h[keep] - cy) / fy * d
    T = np.asarray(t_wc, np.float32).astype(np.float64)
    pc = np.stack([x, y, d], 1)
    pts = pc @ T[:3, :3].T + T[:3, 3]
    scale = np.abs(pc) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])
    return pts, scale


# ---- extents -----------------------------------------------------------------------------------------------------------------------

def centred32(points, center=None):
    """What the kernel projects: float32 points minus a float32 centre, rounded to float32; returned as float64."""
    p = np.asarray(points, np.float32)
    if center is not None:
        p = p - np.asarray(center, np.float32)
    return p.astype(np.float64)


def extents64(points, rotations, center=None):
    """lo, hi [K, 3] of the float32-centred points projected on the rows of the float32 ``rotations`` [K, 3, 3], in float64; and the
    bound scale sum_i |q_i r_i| at the two extreme points [K, 3] each."""
    q = centred32(points, center)
    r = np.asarray(rotations, np.float32).astype(np.float64)
    K = len(r)
    lo, hi, slo, shi = (np.zeros((K, 3)) for _ in range(4))
    for k0 in range(0, K, 256):
        rr = r[k0:k0 + 256].reshape(-1, 3)
        proj = q @ rr.T
        mag = np.abs(q) @ np.abs(rr).T
        i_lo, i_hi = proj.argmin(0), proj.argmax(0)
        cols = np.arange(proj.shape[1])
        lo[k0:k0 + 256] = proj[i_lo, cols].reshape(-1, 3)
        hi[k0:k0 + 256] = proj[i_hi, cols].reshape(-1, 3)
        slo[k0:k0 + 256] = mag[i_lo, cols].reshape(-1, 3)
        shi[k0:k0 + 256] = mag[i_hi, cols].reshape(-1, 3)
    return lo, hi, slo, shi


def box_volume_along(points, R_rows):
    p = np.asarray(points, np.float64) @ np.asarray(R_rows, np.float64).T
    return float(np.prod(p.max(0) - p.min(0)))


def exhaustive_search(points, step_deg=2.5):
    """The smallest box volume over a fixed grid of frames (first axis over a hemisphere in ``step_deg`` steps, in-plane angle over
    [0, 90) in the same steps): a slow, dumb comparison for small clouds."""
    p = np.asarray(points, np.float64)
    p = p - p.mean(0)
    step = math.radians(step_deg)
    best = math.inf
    for th in np.arange(0.0, 0.5 * math.pi + 1e-9, step):
        n_phi = max(1, int(round(2 * math.pi * math.sin(th) / step)))
        for phi in np.arange(n_phi) * (2 * math.pi / n_phi):
            a = np.array([math.sin(th) * math.cos(phi), math.sin(th) * math.sin(phi), math.cos(th)])
            h = np.eye(3)[np.argmin(np.abs(a))]
            b0 = np.cross(a, h)
            b0 /= np.linalg.norm(b0)
            c0 = np.cross(a, b0)
            ea = np.ptp(p @ a)
            pb, pc = p @ b0, p @ c0
            for psi in np.arange(0.0, 0.5 * math.pi, step):
                u = math.cos(psi) * pb + math.sin(psi) * pc
                v = -math.sin(psi) * pb + math.cos(psi) * pc
                best = min(best, ea * np.ptp(u) * np.ptp(v))
    return best


# ---- analytic clouds ---------------------------------------------------------------------------------------------------------------

def box_cloud(extent, n, rng, R=None, center=(0, 0, 0)):
    """n uniform points inside a box of full ``extent`` plus its 8 corners, rotated by R (columns = box axes) and moved to center."""
    e = np.asarray(extent, np.float64)
    corners = np.array([[sx, sy, sz] for sx in (-.5, .5) for sy in (-.5, .5) for sz in (-.5, .5)]) * e
    p = np.concatenate([corners, (rng.random((n, 3)) - 0.5) * e])
    R = np.eye(3) if R is None else R
    return p @ R.T + np.asarray(center, np.float64)


def l_shape_cloud(n, rng, R=None, center=(0, 0, 0)):
    """Two 3 x 1 x 1 bars forming an L in the plane z in [0, 1] (with their corners): its axis-aligned box is 3 x 3 x 1."""
    a = box_cloud((3, 1, 1), n // 2, rng, center=(1.5, 0.5, 0.5))
    b = box_cloud((1, 3, 1), n - n // 2, rng, center=(0.5, 1.5, 0.5))
    p = np.concatenate([a, b])
    R = np.eye(3) if R is None else R
    return p @ R.T + np.asarray(center, np.float64)


def tetrahedron_cloud(n, rng, R=None, center=(0, 0, 0)):
    """A regular tetrahedron inscribed in the unit cube (alternate corners; edge sqrt 2) with its vertices: the cube, volume 1, is its
    minimum-volume box (O'Rourke 1985 uses it as the example of a minimum box flush with no face)."""
    v = np.array([[0, 0, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1]], np.float64) - 0.5
    w = rng.dirichlet(np.ones(4), n)
    p = np.concatenate([v, w @ v])
    R = np.eye(3) if R is None else R
    return p @ R.T + np.asarray(center, np.float64)


def volume_inflation(extent, theta):
    """prod_i (1 + theta (e_j + e_k) / e_i): how much a box of extents e can grow when measured in a frame off by theta radians."""
    e = np.asarray(extent, np.float64)
    return float(np.prod([1 + theta * (e.sum() - e[i]) / e[i] for i in range(3)]))


# ---- box conditions ----------------------------------------------------------------------------------------------------------------

def box_violations(box, points, min_extent=0.10):
    """A list of the conditions a returned box breaks on ``points`` (empty = all hold), checked in float64: containment
    |R^T (p - c)| <= extent / 2 + 2^-20 max |p - c|, R orthonormal to 1e-6 with det > 0, extents ascending and >= min_extent."""
    p = np.asarray(points, np.float64)
    c, R, e = np.asarray(box.center, np.float64), np.asarray(box.R, np.float64), np.asarray(box.extent, np.float64)
    bad = []
    q = p - c
    tol = 2.0 ** -20 * np.abs(q).max()
    over = (np.abs(q @ R) - (e / 2 + tol)).max()
    if over > 0:
        bad.append(f"containment exceeded by {over:.3e} (tol {tol:.3e})")
    if np.abs(R.T @ R - np.eye(3)).max() > 1e-6:
        bad.append(f"R not orthonormal: {np.abs(R.T @ R - np.eye(3)).max():.3e}")
    if not np.linalg.det(R) > 0:
        bad.append("det R <= 0")
    if np.any(np.diff(e) < 0):
        bad.append(f"extents not ascending: {e}")
    if e.min() < min_extent:
        bad.append(f"extent below {min_extent}: {e}")
    return bad


# ---- the scene ---------------------------------------------------------------------------------------------------------------------

class Scene:
    """Boxes (centre, R with axes as columns, full extent, instance id) seen by ``n_views`` pinhole cameras on a ring of ``radius``
    around the origin looking at it, alternating above and below the ring's plane so that every face is seen.  Depth by exact
    ray / box intersection in float64 (z-depth along the optical axis), instance image from the hit test.  Around it: a background
    of instance 0 at a constant depth, and inside the objects some pixels relabelled -1 (unknown) and some with depth 0 - all of
    which the unprojection must ignore.  Frames are stored [W, H] like the package's keyframes."""

    def __init__(self, width=160, height=120, fx=150.0, n_views=10, radius=3.0, seed=0):
        self.W, self.H, self.k4 = width, height, (fx, fx, (width - 1) / 2.0, (height - 1) / 2.0)
        self.radius = radius
        self.boxes = [dict(id=3, center=np.array([-0.75, 0.05, 0.0]), R=rotation((1, 2, 3), 0.6), extent=np.array([0.6, 0.9, 1.5])),
                      dict(id=7, center=np.array([0.85, -0.05, 0.05]), R=rotation((-2, 1, 1), 1.1), extent=np.array([1.0, 1.0, 1.0]))]
        rng = np.random.default_rng(seed)
        self.frames = []
        for v in range(n_views):
            az = 2 * math.pi * v / n_views
            el = math.radians(35.0) * (1 if v % 2 == 0 else -1)
            pos = radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
            z = -pos / np.linalg.norm(pos)
            x = np.cross(z, np.array([0.0, 0.0, 1.0]))
            x /= np.linalg.norm(x)
            y = np.cross(z, x)
            t_wc = np.eye(4)
            t_wc[:3, 0], t_wc[:3, 1], t_wc[:3, 2], t_wc[:3, 3] = x, y, z, pos
            self.frames.append(self._render(t_wc, rng))

    def _render(self, t_wc, rng):
        fx, fy, cx, cy = self.k4
        w, h = np.meshgrid(np.arange(self.W), np.arange(self.H), indexing="ij")
        dirs_c = np.stack([(w - cx) / fx, (h - cy) / fy, np.ones_like(w, np.float64)], -1)          # z component 1: t = z-depth
        dirs_w = dirs_c @ t_wc[:3, :3].T
        o = t_wc[:3, 3]
        depth = np.full((self.W, self.H), 6.0)
        inst = np.zeros((self.W, self.H), np.int32)
        best = np.full((self.W, self.H), np.inf)
        for b in self.boxes:
            ob = (o - b["center"]) @ b["R"]
            db = dirs_w @ b["R"]
            with np.errstate(divide="ignore", invalid="ignore"):
                t1 = (-b["extent"] / 2 - ob) / db
                t2 = (b["extent"] / 2 - ob) / db
            tn = np.minimum(t1, t2).max(-1)
            tf = np.maximum(t1, t2).min(-1)
            hit = (tn <= tf) & (tn > 0) & (tn < best)
            best = np.where(hit, tn, best)
            depth = np.where(hit, tn, depth)
            inst = np.where(hit, b["id"], inst)
        obj = inst > 0
        u = rng.random((self.W, self.H))
        inst = np.where(obj & (u < 0.02), -1, inst)                      # unknown pixels
        depth = np.where(obj & (u > 0.98), 0.0, depth)                   # holes in the depth image
        return dict(depth=depth.astype(np.float32), inst=inst.astype(np.int32), t_wc=t_wc.astype(np.float32))

    def cloud(self, obj_id, frames=None):
        """(points [n, 3], scale [n, 3]) of one object over the frames (default all), in (frame, pixel) order, float64."""
        parts = [unproject(f["depth"], f["inst"], f["t_wc"], self.k4, obj_id) for f in (self.frames if frames is None else frames)]
        return np.concatenate([p for p, _ in parts]), np.concatenate([s for _, s in parts])

    def footprint(self):
        return self.radius / self.k4[0]
