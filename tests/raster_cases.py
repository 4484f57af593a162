"""Scenes of the rasteriser tests (tests/test_raster.py on the CPU, tests/test_gpu_raster.py on the device): random triangle soups
with every kind of face the contract drops, the coarse sphere-over-plane scene of the geometric test, the lattice scene whose snapped
vertices fall on pixel centres, and a box room seen from inside.  Poses are [K, 4, 4] camera to world; images [K, W, H]."""
from __future__ import annotations

import numpy as np

import cull_cases as cc

f32 = np.float32
SETUP_WG = 256                                 # vr::kRasterWG: faces per block of the setup pass


def random_scene(width, height, n_faces, K, seed=0, spare_slots=1):
    """(vertices [3 n_faces + 1, 3], faces [n_faces, 3], t_wc [K + spare_slots, 4, 4], intrinsics).  Cameras on cull_cases' ring of
    radius 3 around the origin; triangles of 0.05 .. 2.5 m (most of them small) somewhere in a 5 m cube, so that some are a pixel wide and some cover many
    tiles, some lie behind a camera and some straddle its near plane.  Deliberate faces: 0 has a NaN vertex, 1 an index out of range
    (and 2 a negative one), 3 lies wholly behind camera 0, 4 has a corner outside camera 0's guard band; the spare poses are all zero."""
    rng = np.random.default_rng(seed)
    _, _, t_wc, intr = cc.random_scene(width, height, 1, K, seed=seed, spare_slots=spare_slots)
    centre = (rng.random((n_faces, 1, 3)) - 0.5) * 5.0
    size = 0.05 + 2.5 * rng.random((n_faces, 1, 1)) ** 3
    tri = (centre + (rng.random((n_faces, 3, 3)) - 0.5) * size).astype(np.float32)
    faces = np.arange(3 * n_faces, dtype=np.int32).reshape(n_faces, 3)
    flip = rng.random(n_faces) < 0.5
    faces[flip] = faces[flip][:, [0, 2, 1]]                                   # both windings
    R, t = t_wc[0, :3, :3].astype(np.float64), t_wc[0, :3, 3].astype(np.float64)
    tri[0, 1] = [np.nan, 0.1, 0.2]
    tri[3] = (t + (R @ np.array([[0.1, 0.0, -1.0], [0.3, 0.1, -1.2], [0.0, 0.3, -1.1]]).T).T).astype(np.float32)
    tri[4] = (t + (R @ np.array([[0.0, 0.0, 1.0], [0.1, 0.1, 1.0], [100.0, 0.0, 0.06]]).T).T).astype(np.float32)
    vertices = np.concatenate([tri.reshape(-1, 3), np.zeros((1, 3), np.float32)])
    faces[1, 2] = len(vertices)                                               # one past the last vertex
    faces[2, 0] = -1
    return vertices, faces, t_wc, intr


def uv_sphere(n_lat, n_lon, radius, centre):
    """(vertices, faces): a latitude / longitude grid of (n_lat + 1) x n_lon vertices, two triangles per cell - the cells at the poles
    have a zero-area triangle each, deliberately."""
    th = np.linspace(0.0, np.pi, n_lat + 1)
    ph = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing="ij")
    v = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3) * radius + np.asarray(centre)
    idx = np.arange((n_lat + 1) * n_lon).reshape(n_lat + 1, n_lon)
    a, b = idx[:-1], idx[1:]
    an, bn = np.roll(a, -1, 1), np.roll(b, -1, 1)
    faces = np.concatenate([np.stack([a, b, bn], -1).reshape(-1, 3), np.stack([a, bn, an], -1).reshape(-1, 3)])
    return v, faces


def grid_plane(nx, ny, x0, x1, y0, y1, z):
    gx, gy = np.meshgrid(np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1), indexing="ij")
    v = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], 1)
    idx = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])


GEO_W, GEO_H = 96, 72
GEO_INTRINSICS = (80.0, 80.0, 47.5, 35.5)
GEO_MIN_DEPTH = 0.05


def sphere_plane_scene():
    """The coarse scene of the geometric test: a UV sphere of 8 x 10 segments, radius 0.5 at (0.2, 0, 1.6), in front of a 7 x 5-cell
    plane over x in [-2, 2], y in [-1.5, 1.5] at z = 2.5 - 160 + 70 = 230 faces; the camera rotated 0.3 rad about y, then 0.2 rad about
    x, at (0.1, -0.05, -0.2).  -> (vertices float32, faces int32, t_wc [1, 4, 4])"""
    sv, sf = uv_sphere(8, 10, 0.5, (0.2, 0.0, 1.6))
    pv, pf = grid_plane(7, 5, -2.0, 2.0, -1.5, 1.5, 2.5)
    vertices = np.concatenate([sv, pv]).astype(np.float32)
    faces = np.concatenate([sf, pf + len(sv)]).astype(np.int32)
    assert len(faces) == 230
    R = cc.rotation([1, 0, 0], 0.2) @ cc.rotation([0, 1, 0], 0.3)
    return vertices, faces, cc.pose(R, [0.1, -0.05, -0.2])[None]


# ---- the lattice scene: identity pose, fx = fy = 10, cx = cy = 0, z = 1: a vertex (0.1 i, 0.1 j, 1) projects to the pixel centre (i, j)
LAT_INTRINSICS = (10.0, 10.0, 0.0, 0.0)
LAT_W, LAT_H = 12, 10
IDENT = np.eye(4, dtype=np.float32)[None]


def lattice_scene(x0=2, x1=8, y0=2, y1=6, z=1.0):
    """A grid of 2-pixel cells over the pixel rectangle [x0, x1] x [y0, y1] (vertices at multiples of 0.2 m = 2 pixels), every cell split
    along alternating diagonals, the faces in both windings."""
    nx, ny = (x1 - x0) // 2, (y1 - y0) // 2
    v, _ = grid_plane(nx, ny, 0.1 * x0, 0.1 * x1, 0.1 * y0, 0.1 * y1, z)
    idx = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    faces = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = idx[i, j], idx[i + 1, j], idx[i + 1, j + 1], idx[i, j + 1]
            faces += [[a, b, c], [a, d, c]] if (i + j) % 2 == 0 else [[a, b, d], [b, d, c]]
    return v.astype(np.float32), np.array(faces, np.int32)


def box_room(half=(2.0, 1.5, 2.5)):
    """(vertices, faces): the 12 triangles of a box around the origin, seen from inside."""
    hx, hy, hz = half
    v = np.array([[x, y, z] for x in (-hx, hx) for y in (-hy, hy) for z in (-hz, hz)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def room_intrinsics(width, height):
    """A long lens (half the image width spans atan(1 / 4)): see room_poses."""
    return (2.0 * width, 2.0 * width, (width - 1) / 2 + 0.25, (height - 1) / 2 - 0.125)


def room_poses():
    """Three poses inside the room.  There is no near-plane clipping: a wall with a corner behind the camera is dropped whole, and from
    inside a box that is every wall the camera does not face.  So each pose looks, through room_intrinsics' long lens, at walls that
    lie wholly in front of it and fill the image: into a vertical edge of the room along a diagonal (two walls, four faces and the
    edge between them), the same from the opposite side with a roll, and straight at one wall."""
    return np.stack([cc.pose(cc.rotation([0, 1, 0], np.pi / 4) @ cc.rotation([0, 0, 1], 0.1), [-1.5, 0.0, -2.0]),
                     cc.pose(cc.rotation([0, 1, 0], np.pi / 4 + np.pi) @ cc.rotation([0, 0, 1], -0.2), [1.4, 0.1, 1.9]),
                     cc.pose(cc.rotation([1, 0, 0], 0.03), [0.2, 0.1, -2.0])])
