"""Scenes of the visibility-culling tests (tests/test_cull.py on the CPU, tests/test_gpu_cull.py on the device): a random scene whose
decisions stay clear of their boundaries for all but a few points, the deliberate boundary cases of the contract, and a known-answer
scene - a wall and a small box behind it.  Depth images are [K, W, H], width-major."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def rotation(axis, angle):
    """Rodrigues, float64."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(np.float32)


def intrinsics_for(width, height):
    return (float(width) * 0.9, float(width) * 0.95, (width - 1) / 2 + 0.25, (height - 1) / 2 - 0.125)


def random_scene(width, height, n, K, seed=0, spare_slots=0):
    """(points [n, 3], depth [K + spare_slots, W, H], t_wc [K + spare_slots, 4, 4], intrinsics): cameras on a ring of radius 3 looking
    at the origin with a real rotation each, points in a 5 m cube around it (some behind a camera, some outside every frustum),
    depth images of random values around the distance to the origin with holes (0) - so the occlusion decision falls either way - and
    the spare slots all zero, as unused slots of a store are."""
    rng = np.random.default_rng(seed)
    pts = ((rng.random((n, 3)) - 0.5) * 5.0).astype(np.float32)
    t_wc = np.zeros((K + spare_slots, 4, 4), np.float32)
    for k in range(K):
        ang = 2 * np.pi * k / max(K, 1) + 0.3
        eye = np.array([3 * np.cos(ang), 0.4 * np.sin(3 * ang), 3 * np.sin(ang)])
        zc = -eye / np.linalg.norm(eye)                            # the optical axis: towards the origin
        xc = np.cross([0.0, 1.0, 0.0], zc)
        xc /= np.linalg.norm(xc)
        R = np.stack([xc, np.cross(zc, xc), zc], 1) @ rotation([0, 0, 1], 0.2 * k)     # columns = the camera's axes, rolled
        t_wc[k] = pose(R, eye)
    depth = np.zeros((K + spare_slots, width, height), np.float32)
    depth[:K] = (3.0 + (rng.random((K, width, height)) - 0.5) * 2.0).astype(np.float32)
    depth[:K][rng.random((K, width, height)) < 0.1] = 0.0
    return pts, depth, t_wc, intrinsics_for(width, height)


# ---- the known-answer scene ---------------------------------------------------------------------------------------------------------
WALL_Z, BOX_Z = 3.0, (3.5, 4.0)
KA_W, KA_H = 64, 48
KA_INTRINSICS = (60.0, 60.0, 31.5, 23.5)
KA_EPS = 0.05


def known_answer_scene():
    """A wall in the plane z = 3 (a 17 x 17 grid of vertices over [-4, 4]^2, wider than every frustum) and a small box 0.5 m behind
    it, seen from three poses in front of the wall (one rotated about y, one about x); the depth images are the analytic ray-plane
    intersection with the wall, pixel by pixel.  -> dict(vertices, faces, n_wall, depth, t_wc)"""
    g = np.linspace(-4.0, 4.0, 17) + 0.013                         # off every image edge and every rounding tie
    gx, gy = np.meshgrid(g, g, indexing="ij")
    wall = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, WALL_Z)], 1)
    idx = np.arange(17 * 17).reshape(17, 17)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    wall_faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    corners = np.array([[x, y, z] for x in (-0.3, 0.3) for y in (-0.25, 0.25) for z in BOX_Z])
    box_faces = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    poses = [pose(np.eye(3), [0.0, 0.0, 0.0]), pose(rotation([0, 1, 0], 0.15), [-0.5, 0.1, 0.2]), pose(rotation([1, 0, 0], -0.1), [0.37, -0.2, -0.3])]
    t_wc = np.stack(poses)
    fx, fy, cx, cy = KA_INTRINSICS
    w, h = np.meshgrid(np.arange(KA_W), np.arange(KA_H), indexing="ij")
    depth = np.zeros((3, KA_W, KA_H), np.float32)
    for k, T in enumerate(t_wc.astype(np.float64)):
        dirs = np.stack([(w - cx) / fx, (h - cy) / fy, np.ones_like(w, np.float64)], -1) @ T[:3, :3].T      # world directions, camera z = 1
        depth[k] = ((WALL_Z - T[2, 3]) / dirs[..., 2]).astype(np.float32)                                  # = depth along the optical axis
    return dict(vertices=np.concatenate([wall, corners]).astype(np.float32), faces=np.concatenate([wall_faces, box_faces + len(wall)]).astype(np.int32),
                n_wall=len(wall), depth=depth, t_wc=t_wc)


def random_faces(n_vertices, n_faces, seed=0):
    """int32 [n_faces, 3] with a few faces that repeat an index."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, n_vertices, (n_faces, 3)).astype(np.int32)
    rep = rng.random(n_faces) < 0.05
    f[rep, 1] = f[rep, 0]
    return f
