"""TEST INFRASTRUCTURE: the scenes of the depth tracker's tests.  Everything is analytic and ray-cast in numpy: a room corner of three
planes (x = 0, y = 0, z = 0, the room in the positive octant) with a sphere in front of it, seen from poses that are known exactly.
Nothing comes from outside."""
import numpy as np

import icp_oracle as io

SPHERE_CENTER = np.array([0.55, 0.6, 0.5])
SPHERE_RADIUS = 0.35
EYE = np.array([2.1, 1.7, 1.5])


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """Camera-to-world [4, 4] float64: z looks from eye to target, x to the right, y down."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


def intrinsics_for(width, height):
    """A 56-degree horizontal field of view whatever the size, the principal point at the image centre."""
    f = 0.94 * width
    return (f, f, (width - 1) / 2.0, (height - 1) / 2.0)


def render(t_wc, intrinsics, width, height, sphere=True, planes=(0, 1, 2)):
    """Depth along the optical axis, float32 [W, H]; 0 where a ray hits nothing."""
    fx, fy, cx, cy = intrinsics
    w, h = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64), indexing="ij")
    d_cam = np.stack([(w - cx) / fx, (h - cy) / fy, np.ones_like(w)], -1)
    d = d_cam @ t_wc[:3, :3].T
    o = t_wc[:3, 3]
    best = np.full((width, height), np.inf)
    with np.errstate(all="ignore"):
        for k in planes:
            t = -o[k] / d[..., k]
            hit = o + t[..., None] * d
            ok = (t > 0) & (hit >= -1e-9).all(-1)
            best = np.where(ok & (t < best), t, best)
        if sphere:
            oc = o - SPHERE_CENTER
            a, b, c = (d * d).sum(-1), 2 * (d * oc).sum(-1), oc @ oc - SPHERE_RADIUS ** 2
            disc = b * b - 4 * a * c
            t = (-b - np.sqrt(disc)) / (2 * a)
            best = np.where((disc > 0) & (t > 0) & (t < best), t, best)
    return np.where(np.isfinite(best), best, 0.0).astype(np.float32)


def offset(trans, angle_deg, axis=(0.3, -0.5, 0.8)):
    """A rigid motion [4, 4]: `angle_deg` about `axis`, and a translation of length `trans` metres."""
    axis = np.asarray(axis, np.float64)
    T = np.eye(4)
    T[:3, :3] = io.rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(angle_deg))
    t = np.array([0.6, 0.3, -0.74])
    T[:3, 3] = t / np.linalg.norm(t) * trans
    return T


def rigid_inverse(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def corner_scene(width, height, trans=0.02, angle_deg=1.0, **kw):
    """The model seen from EYE, the source from EYE moved by (trans, angle_deg) in the camera frame.  -> dict: depth, model_depth
    [W, H] float32, t_wc_model, t_wc_true [4, 4] float64, intrinsics, T_true [12] (source camera -> model camera)."""
    intr = intrinsics_for(width, height)
    t_model = look_at(EYE)
    t_true = t_model @ offset(trans, angle_deg)
    return dict(depth=render(t_true, intr, width, height, **kw), model_depth=render(t_model, intr, width, height, **kw),
                t_wc_model=t_model, t_wc_true=t_true, intrinsics=intr, T_true=(rigid_inverse(t_model) @ t_true)[:3].reshape(12),
                T_init=np.eye(4)[:3].reshape(12))


def corner_mesh(extent=3.0, n=30, rings=20, sectors=32):
    """The scene as small triangles, the way a marching-cubes mesh holds it: the three walls as n x n quads over [0, extent]^2 and the
    sphere as a latitude / longitude grid.  -> (vertices float32 [V, 3], faces int32 [F, 3])"""
    verts, faces = [], []

    def grid(points, rows, cols):
        base = sum(len(v) for v in verts)
        verts.append(points.reshape(-1, 3))
        i, j = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
        a = (base + i * cols + j).reshape(-1)
        faces.append(np.stack([a, a + 1, a + cols], -1))
        faces.append(np.stack([a + 1, a + cols + 1, a + cols], -1))

    u, v = np.meshgrid(np.linspace(0, extent, n + 1), np.linspace(0, extent, n + 1), indexing="ij")
    zero = np.zeros_like(u)
    for k in range(3):
        comps = [u, v]
        comps.insert(k, zero)
        grid(np.stack(comps, -1), n + 1, n + 1)
    th, ph = np.meshgrid(np.linspace(0, np.pi, rings + 1), np.linspace(0, 2 * np.pi, sectors + 1), indexing="ij")
    grid(SPHERE_CENTER + SPHERE_RADIUS * np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1), rings + 1, sectors + 1)
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32)


ITERATIONS = (4, 5, 10)                       # per level index (0 = finest): the public default (10, 5, 4), coarse first
PARAMS = io.Params()

# Convergence on corner_scene(64, 48) from the 2 cm / 1 degree offset, measured on the CPU with tests/icp_oracle.py (pose_error, the
# Frobenius distance of rows 0 .. 2 to T_true); tests/test_icp.py re-measures them and holds the recorded figures to 1 %.
INITIAL_ERROR = 3.176821e-2
PLAIN_ERROR = 6.577196e-4
EXACT_ERROR = 6.576561e-4
EXACT_OVER_PLAIN = 0.999903
