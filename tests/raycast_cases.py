"""TEST INFRASTRUCTURE: the scenes and the measured constants of the TSDF ray cast's tests.  Everything is analytic or drawn from seeded
generators: tsdf_cases' room corner with a sphere fused by the numpy checker, and volumes prefilled with noise.  Nothing comes from
outside, and nothing can be held against an outside implementation."""
import functools

import numpy as np

import icp_cases as ic
import raycast_oracle as ro
import tsdf_cases as tc
import tsdf_oracle as to

f32 = np.float32

# ---- the bit-equality scenes -------------------------------------------------------------------------------------------------------------
SHAPES = {"19x26x33": ((19, 26, 33), "grid"), "2x9x17": ((2, 9, 17), "grid"), "5x9x70": ((5, 9, 70), "oriented")}
IMAGES = ((37, 29), (64, 48))
STATES = ("fused", "noise")
TRUNC = 0.2
KW = dict(min_depth=0.1, max_depth=tc.MAX_DEPTH, min_weight=1.0, step=TRUNC / 2, max_steps=4096)


def affine_of(shape, kind):
    if kind == "oriented":
        return tc.oriented_affine()
    s = 1.5 / (max(shape) - 1)
    return np.array([[s, 0, 0, tc.LO], [0, s, 0, tc.LO], [0, 0, s, tc.LO]])


@functools.lru_cache(maxsize=None)
def volume(name, state):
    """-> (vol dict float32 with colour, shape, affine).  'fused': the exact checker's fusion of tsdf_cases.many_frames (dirty depth, an
    unused slot); 'noise': tsdf_cases.prefilled - crossings, holes and back faces everywhere."""
    shape, kind = SHAPES[name]
    A = affine_of(shape, kind)
    if state == "noise":
        return tc.prefilled(shape, True, 11), shape, A
    sc = tc.many_frames(64, 48, 5, seed=3)
    vol = to.integrate_f32(to.empty(shape, True), shape, A, sc["depth"], sc["t_wc"], sc["intrinsics"], rgbx=sc["rgbx"], trunc=TRUNC,
                           max_depth=tc.MAX_DEPTH)
    return vol, shape, A


def views_of(shape, A):
    """Three poses [3, 4, 4] float64: an eye outside looking at the scene, an all-zero slot, and an eye INSIDE the volume."""
    A = np.asarray(A, np.float64)
    at = lambda frac: A[:, :3] @ ((np.array(shape) - 1) * np.asarray(frac)) + A[:, 3]
    inside = ic.look_at(at((0.6, 0.55, 0.7)), at((0.1, 0.2, 0.15)))
    return np.stack([ic.look_at((2.1, 1.7, 1.5), tc.TARGET), np.zeros((4, 4)), inside])


def pack_host_input(shape, vol, M32, N32, intrinsics, width, height, *, min_depth, max_depth, min_weight, step, max_steps):
    """The input file of tests/tools/raycast_rules_host.cpp as bytes."""
    color = vol["color"] is not None
    head = np.array(list(shape) + [width, height, max_steps, len(M32), int(color)], np.int32)
    fl = np.concatenate([np.asarray(intrinsics, np.float64), [min_depth, max_depth, step, min_weight], np.asarray(N32, np.float64).reshape(9)]).astype(f32)
    parts = [head, fl, np.asarray(M32, f32), vol["tsdf"].astype(f32), vol["weight"].astype(f32)] + ([vol["color"].astype(f32)] if color else [])
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


def unpack_host_output(data, shape, K, width, height, color):
    """-> (classes uint8 [bx, by, bz], plain, classed): the two dicts hold depth, status, normal and color (or None)."""
    bd = tuple(ro.brick_dim(s) for s in shape)
    nb, P = int(np.prod(bd)), K * width * height
    classes = np.frombuffer(data, np.uint8, nb).reshape(bd)
    off, forms = nb, []
    for _ in range(2):
        d = np.frombuffer(data, f32, P, off).reshape(K, width, height); off += 4 * P
        s = np.frombuffer(data, np.uint8, P, off).reshape(K, width, height); off += P
        n = np.frombuffer(data, f32, 3 * P, off).reshape(K, width, height, 3); off += 12 * P
        c = None
        if color:
            c = np.frombuffer(data, np.uint8, 4 * P, off).reshape(K, width, height, 4); off += 4 * P
        forms.append(dict(depth=d, status=s, normal=n, color=c))
    assert off == len(data)
    return classes, forms[0], forms[1]


def same_bits(a, b, keys=("depth", "status", "normal", "color")):
    """The keys on which two results differ in some bit (a float compared as its bits: -0 is not 0, a NaN equals itself)."""
    bad = []
    for key in keys:
        x, y = a[key], b[key]
        if x is None or y is None:
            if (x is None) != (y is None):
                bad.append(key)
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(key)
    return bad


# ---- the geometry scene of the issue: tsdf_cases' 32^3 volume fused from its four EYES by the plain layer, ray-cast from three eyes -----
GEOMETRY_EYES = ((1.8, 1.8, 1.6), (2.1, 1.7, 1.5), (1.4, 2.0, 2.0))
EDGE_SPAN_VOXELS = 3.0                     # a pixel is excluded when its 3 x 3 neighbourhood in the analytic depth image spans more, along the ray
# the issue's caps (conditions, not measurements)
MAX_EXCLUDED, MIN_COMPARED, MAX_SHARE_BEYOND_HALF, MAX_WORST_VOXELS = 0.20, 0.60, 0.02, 1.5
# Measured on the CPU with raycast_oracle's plain (float64) layer, per eye (tests/test_raycast.py re-measures and holds them to these):
# the share of pixels excluded as depth edges, the share hit and compared, of those the share off by more than half a voxel along the
# ray, and the worst error in voxels.
PLAIN_EXCLUDED = (0.0573, 0.0592, 0.1364)
PLAIN_COMPARED = (0.8496, 0.8092, 0.6722)
PLAIN_SHARE_BEYOND_HALF = (0.0015, 0.0024, 0.0039)
PLAIN_WORST_VOXELS = (0.673, 0.812, 0.758)
# the exact (float32) and the plain layer: the same pixels hit, the largest depth difference measured between them, in metres; the
# test allows twice that
EXACT_PLAIN_MAX_DIFF = 1.9552e-6
# normals at the hits outside tsdf_cases.excluded's one-voxel rule: the smallest dot product with tsdf_cases.outward measured on the plain
# layer, and the share of hits the rule excludes (capped at tsdf_cases.MAX_EXCLUDED_SHARE); the test requires at least the bound the
# mesh normals are held to, tsdf_cases.MIN_DOT_OUTSIDE_RULE.  A hit whose normal the contract refuses (one of the six samples at p* +- 1
# voxel is invalid or outside) has no direction to compare: 6.7 % of the hits, every one of them within REFUSED_REACH voxels (Chebyshev)
# of a voxel below min_weight or of the volume's faces - the test holds each refusal to that, and the share to twice the measured one.
PLAIN_MIN_DOT = 0.9237
NORMALS_EXCLUDED_SHARE = 0.0614
NORMALS_REFUSED_SHARE = 0.0674
REFUSED_REACH = 3
# the depth tracker against the exact layer's raycast of the volume (CPU path: raycast_oracle exact at the model pose, then
# icp_oracle.track from icp_cases.offset(0.02, 1.0)): the factor by which the pose error falls below icp_cases.INITIAL_ERROR
TRACK_FACTOR = 12.19


@functools.lru_cache(maxsize=None)
def geometry_volumes():
    """-> (plain volume float64, exact volume float32, shape, affine): the tsdf_cases scene fused by both layers of tsdf_oracle."""
    sc, shape, A = tc.scene(), (tc.GRID,) * 3, tc.grid_affine()
    kw = dict(trunc=tc.TRUNC, max_depth=tc.MAX_DEPTH)
    plain = to.integrate_f64(to.empty(shape, dtype=np.float64), shape, A, sc["depth"], sc["t_wc"], sc["intrinsics"], **kw)
    exact = to.integrate_f32(to.empty(shape), shape, A, sc["depth"], sc["t_wc"], sc["intrinsics"], **kw)
    return plain, exact, shape, A


GEOMETRY_KW = dict(min_depth=0.1, max_depth=tc.MAX_DEPTH, min_weight=1.0, step=tc.TRUNC / 2, max_steps=4096)


def edge_mask(depth):
    """True where the 3 x 3 neighbourhood of the analytic depth image [W, H] (0 = nothing) spans more than EDGE_SPAN_VOXELS along the
    ray, or touches a pixel that sees nothing."""
    W, H = depth.shape
    fx, fy, cx, cy = ic.intrinsics_for(W, H)
    w, h = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    length = np.sqrt(((w - cx) / fx) ** 2 + ((h - cy) / fy) ** 2 + 1)
    pad = np.pad(depth.astype(np.float64), 1, mode="edge")
    stack = np.stack([pad[1 + a:1 + a + W, 1 + b:1 + b + H] for a in (-1, 0, 1) for b in (-1, 0, 1)])
    return ((stack.max(0) - stack.min(0)) * length > EDGE_SPAN_VOXELS * tc.VOXEL) | (stack.min(0) <= 0)
