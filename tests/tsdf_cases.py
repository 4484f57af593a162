"""TEST INFRASTRUCTURE: the scenes of the TSDF fusion tests.  Everything is analytic: icp_cases' room corner with a sphere, ray-cast in
numpy from poses that are known exactly, with instance labels re-derived from which primitive a ray hit and a colour image that is a
function of the pixel.  Nothing comes from outside."""
import numpy as np

import icp_cases as ic
import tsdf_oracle as to

f32 = np.float32

# ---- the geometry scene of the issue: a 32^3 grid over [-0.15, 1.35]^3, trunc of 4 voxels, 64 x 48 images from four eyes ------------
GRID = 32
LO, HI = -0.15, 1.35
VOXEL = (HI - LO) / (GRID - 1)
TRUNC = 4 * VOXEL
EYES = ((2.1, 1.7, 1.5), (1.5, 2.2, 1.2), (2.3, 1.0, 1.9), (1.2, 1.4, 2.4))
TARGET = (0.4, 0.4, 0.4)
WIDTH, HEIGHT = 64, 48
SPHERE_ID, WALL_ID = 1, 2
MAX_DEPTH = 10.0

# Measured on the CPU with tsdf_oracle's plain (float64) layer on this scene (tests/test_tsdf.py re-measures and holds them to these):
# masked-mesh vertices, the share of them farther than half a voxel from the true surface min(x, y, z, |p - c| - r), and the worst
# distance in voxels.  The issue's caps: >= 3000 vertices, <= 2 % beyond half a voxel, none beyond 1.5 voxels.
PLAIN_VERTICES = 4104
PLAIN_SHARE_BEYOND_HALF = 0.0041
PLAIN_WORST_VOXELS = 0.98
MIN_VERTICES, MAX_SHARE_BEYOND_HALF, MAX_WORST_VOXELS = 3000, 0.02, 1.5
# the exact (float32) and the plain layer: the same vertex set, the largest coordinate difference measured between them, in metres;
# the test allows twice that
EXACT_PLAIN_MAX_DIFF = 4.4585e-5
# normals: the share of vertices the one-voxel rule excludes (the sphere's silhouettes and the creases), measured; the issue's cap is
# 25 %.  Outside the rule the smallest dot product of a vertex normal with the analytic direction is 0.617 (both layers), and every face
# agrees with its three vertex normals.  Inside it the checker's own mesh has 4 of 7687 faces (8 of 23061 corners) that disagree, all at
# the 90-degree wall creases, where a vertex carries one wall's normal and the face lies on the other wall: the sign is not defined there.
EXCLUDED_SHARE = 0.1664
MAX_EXCLUDED_SHARE = 0.25
MIN_DOT_OUTSIDE_RULE = 0.617
# the depth tracker on the exact layer's mesh, CPU path (raster_oracle.raster_f32 at the model pose, icp_oracle.track from
# icp_cases.offset(0.02, 1.0)): the factor by which the pose error falls below icp_cases.INITIAL_ERROR; the device must reach half of it
TRACK_FACTOR = 19.0


def grid_affine(grid=GRID, lo=LO, hi=HI):
    s = (hi - lo) / (grid - 1)
    return np.array([[s, 0, 0, lo], [0, s, 0, lo], [0, 0, s, lo]], np.float64)


def oriented_affine():
    """A rotated, anisotropic affine whose box still covers the scene's corner and sphere."""
    R = ic.io.rodrigues(np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8]) * np.deg2rad(25.0))
    A = R * np.array([0.07, 0.11, 0.023])[None, :]
    return np.concatenate([A, (np.array([0.5, 0.5, 0.4]) - A @ np.array([4.0, 4.0, 30.0]))[:, None]], 1)


def colour_image(width, height, k):
    """uint8 [W, H, 4]: a function of the pixel and the frame; byte 3 is junk the kernel must not read into the colour."""
    w, h = np.meshgrid(np.arange(width), np.arange(height), indexing="ij")
    return np.stack([(7 * w + 3 * h + 40 * k) % 256, (5 * h + 11 * k) % 256, (w * h + k) % 256, (13 * w + k) % 256], -1).astype(np.uint8)


def labels(t_wc, intrinsics, width, height):
    """int32 [W, H]: SPHERE_ID where the ray hits the sphere first, WALL_ID where it hits a wall first, -1 where it hits nothing -
    re-derived from render: the sphere wins a pixel iff the full scene is nearer there than the walls alone."""
    full = ic.render(t_wc, intrinsics, width, height)
    walls = ic.render(t_wc, intrinsics, width, height, sphere=False)
    sphere = (full > 0) & ((walls == 0) | (full < walls))
    return np.where(sphere, SPHERE_ID, np.where(full > 0, WALL_ID, -1)).astype(np.int32)


def scene(width=WIDTH, height=HEIGHT, eyes=EYES, target=TARGET):
    """-> dict: depth [K, W, H] float32, t_wc [K, 4, 4] float32, intrinsics, inst [K, W, H] int32, rgbx [K, W, H, 4] uint8."""
    intr = ic.intrinsics_for(width, height)
    poses = [ic.look_at(e, target) for e in eyes]
    return dict(depth=np.stack([ic.render(T, intr, width, height) for T in poses]), t_wc=np.stack(poses).astype(f32), intrinsics=intr,
                inst=np.stack([labels(T, intr, width, height) for T in poses]),
                rgbx=np.stack([colour_image(width, height, k) for k in range(len(poses))]))


def dirty(depth, seed):
    """A depth image with a NaN, an inf, a -inf, zeros, a negative value, a value under any min_depth in use and one past max_depth."""
    d = depth.copy()
    rng = np.random.default_rng(seed)
    W, H = d.shape
    for v in (np.nan, np.inf, -np.inf, 0.0, 0.0, -1.0, 0.05, 11.0):
        d[rng.integers(W), rng.integers(H)] = v
    d[W // 2:W // 2 + 3, H // 3:H // 3 + 2] = 0.0
    return d


def many_frames(width, height, n, seed=0):
    """n frames on a ring around the scene (dirty depth), for the K-frame cases; slot 0 is left as an unused FrameStore slot (all zero)."""
    rng = np.random.default_rng(seed)
    eyes = [(1.6 + 0.7 * np.cos(a), 1.6 + 0.7 * np.sin(a), 1.2 + 0.5 * rng.uniform()) for a in np.linspace(0.2, 1.3, n)]
    sc = scene(width, height, eyes)
    sc["depth"] = np.stack([dirty(d, seed + k) for k, d in enumerate(sc["depth"])])
    for key in ("depth", "t_wc", "inst", "rgbx"):
        sc[key][0] = -1 if key == "inst" else 0
    return sc


def true_sdf_parts(p):
    p = np.asarray(p, np.float64)
    return np.concatenate([p, (np.linalg.norm(p - ic.SPHERE_CENTER, axis=1) - ic.SPHERE_RADIUS)[:, None]], 1)


def true_sdf(p):
    """min(x, y, z, |p - c| - r): the scene's surface is its zero set (positive = free space)."""
    return true_sdf_parts(p).min(1)


def outward(p):
    """The analytic direction to free space at the surface nearest to p: a wall's axis or the sphere's radius."""
    p = np.asarray(p, np.float64)
    which = np.abs(true_sdf_parts(p)).argmin(1)
    r = p - ic.SPHERE_CENTER
    d = np.concatenate([np.eye(3), np.zeros((1, 3))])[which]
    return np.where((which == 3)[:, None], r / np.linalg.norm(r, axis=1, keepdims=True), d)


def excluded(p, eyes=EYES, voxel=VOXEL):
    """The one-voxel rule: True where p lies within one voxel of a wall crease (two of the four distances within a voxel of each other
    at the surface) or of the sphere's silhouette as some eye sees it: the circle where the cone of rays tangent to the sphere touches it."""
    p = np.asarray(p, np.float64)
    parts = np.sort(np.abs(true_sdf_parts(p)), 1)
    out = parts[:, 1] - parts[:, 0] < voxel
    for e in eyes:
        e = np.asarray(e, np.float64)
        axis = ic.SPHERE_CENTER - e
        dist = np.linalg.norm(axis)
        alpha = np.arcsin(ic.SPHERE_RADIUS / dist)
        v = p - e
        rng = np.linalg.norm(v, axis=1)
        theta = np.arccos(np.clip(v @ axis / (rng * dist), -1, 1))
        out |= (rng * np.abs(np.sin(theta - alpha)) < voxel) & (np.abs(rng - dist * np.cos(alpha)) < voxel)
    return out


def pack_host_input(shape, affine, sc, *, trunc, max_weight, color, obj_id, slots, margin, min_depth, max_depth, vol):
    """The input file of tests/tools/tsdf_rules_host.cpp as bytes."""
    K, W, H = sc["depth"].shape
    slots = list(range(K)) if slots is None else [int(s) for s in slots]
    has_inst = obj_id is not None and obj_id >= 0
    head = np.array(list(shape) + [obj_id if has_inst else -1, W, H, margin, K, len(slots), int(color), int(has_inst)], np.int32)
    fl = np.concatenate([np.asarray(affine, np.float64).reshape(-1), sc["intrinsics"], [min_depth, max_depth, trunc, max_weight]]).astype(f32)
    parts = [head, fl, np.array(slots, np.int32), np.asarray(sc["t_wc"], f32), np.asarray(sc["depth"], f32)]
    if color:
        parts.append(np.asarray(sc["rgbx"], np.uint8))
    if has_inst:
        parts.append(np.asarray(sc["inst"], np.int32))
    parts += [vol["tsdf"].astype(f32), vol["weight"].astype(f32)] + ([vol["color"].astype(f32)] if color else [])
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


def unpack_host_output(data, n, color):
    a = np.frombuffer(data, f32)
    out = dict(centres=a[:3 * n].reshape(n, 3), tsdf=a[3 * n:4 * n], weight=a[4 * n:5 * n], color=a[5 * n:9 * n].reshape(n, 4) if color else None)
    assert a.size == (9 if color else 5) * n
    return out


def prefilled(shape, color, seed):
    """A volume that already holds something: random D in [-1, 1], integer weights 0 .. 5, colours with their own weights."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    W = rng.integers(0, 6, n).astype(f32)
    vol = dict(tsdf=(rng.uniform(-1, 1, n) * (W > 0)).astype(f32), weight=W, color=None)
    if color:
        wc = rng.integers(0, 6, n).astype(f32)
        vol["color"] = np.concatenate([rng.uniform(0, 255, (n, 3)) * (wc > 0)[:, None], wc[:, None]], 1).astype(f32)
    return vol
