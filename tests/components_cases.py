"""The inputs of the mesh-component tests, shared by the CPU tier (tests/test_components.py) and the GPU tier
(tests/test_gpu_components.py).  Every generator returns (vertices float32 [V, 3], faces int32 [F, 3])."""
from __future__ import annotations

import os
import re

import numpy as np

f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vmap_amd", "csrc")


def geometry(name):
    """The value of `constexpr int <name> = <number>;` in csrc/launch_geometry.h: the tests take the kernels' block and chunk edges
    from where the kernels take them."""
    with open(os.path.join(CSRC, "launch_geometry.h")) as fh:
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), fh.read())
    assert m, name
    return int(m.group(1))


def positions(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def renumber(vertices, faces, perm):
    """The same mesh with vertex v renamed perm[v] (an out-of-range index stays as it is)."""
    perm = np.asarray(perm, np.int64)
    n = len(vertices)
    out_v = np.empty_like(vertices)
    out_v[perm] = vertices
    f = np.asarray(faces, np.int64)
    ok = (f >= 0) & (f < n)
    return out_v, np.where(ok, perm[np.clip(f, 0, max(n - 1, 0))], f).astype(np.int32)


# Two tetrahedra (vertices 0-3; 5-8: the first scaled by 2), vertex 4 referenced by nobody, a face with a repeated index (9, 9, 10)
# and two faces with an index out of range that would otherwise join the tetrahedra.  The answers, written out: the faces of
# the unit tetrahedron have areas 1/2, 1/2, 1/2 and sqrt(3)/2 = 0x3F5DB3D7 in float32 = 14529495 * 2^-24.
HAND_LABELS = [0, 0, 0, 0, 1, 2, 2, 2, 2, 3, 3]
HAND_VERTICES = [4, 1, 4, 2]
HAND_FACES = [4, 0, 4, 1]
_UNIT_TET = 3 * (1 << 39) + 14529495 * (1 << 16)
HAND_AREA_Q = [_UNIT_TET, 0, 4 * _UNIT_TET, 0]


def hand_made():
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    v = np.concatenate([tet, [[9, 9, 9]], 2 * tet + f32(3), [[5, 5, 5], [6, 5, 5]]]).astype(np.float32)
    tf = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int32)
    faces = np.concatenate([tf[:2], [[0, 5, 11]], tf[2:], tf + 5, [[-1, 2, 6]], [[9, 9, 10]]]).astype(np.int32)
    return v, faces


def strip(n_faces, order="ascending", seed=0):
    """A triangle strip: one component; faces (i, i+1, i+2).  order: the vertex numbering along the strip."""
    n = n_faces + 2
    i = np.arange(n_faces)
    faces = np.stack([i, i + 1, i + 2], 1).astype(np.int32)
    v = np.stack([np.arange(n) * 0.5, (np.arange(n) % 2) * 1.0, np.zeros(n)], 1).astype(np.float32)
    perm = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "random": np.random.default_rng(seed).permutation(n)}[order]
    return renumber(v, faces, perm)


def fan(n_faces, hub_high, seed=0):
    """A fan of n_faces triangles around one hub (index V - 1 or 0): one component, every face on the hub."""
    n = n_faces + 2
    rim = np.arange(n_faces + 1) + (0 if hub_high else 1)
    hub = n - 1 if hub_high else 0
    faces = np.stack([np.full(n_faces, hub), rim[:-1], rim[1:]], 1).astype(np.int32)
    return positions(n, seed), faces


def disjoint_triangles(count, extra_vertices=0, seed=0):
    """count separate triangles + extra_vertices unreferenced ones at the end: C = count + extra_vertices."""
    faces = np.arange(3 * count, dtype=np.int32).reshape(count, 3)
    return positions(3 * count + extra_vertices, seed), faces


def disjoint_tetrahedra(count, seed=0):
    tf = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int32)
    faces = (tf[None] + 4 * np.arange(count, dtype=np.int32)[:, None, None]).reshape(-1, 3)
    return positions(4 * count, seed), faces


def random_triples(n_vertices, n_faces, seed):
    rng = np.random.default_rng(seed)
    return positions(n_vertices, seed + 1), rng.integers(0, n_vertices, (n_faces, 3)).astype(np.int32)


def area_edge_cases():
    """Separate triangles (component k = triangle k) with (0, 0, 0), (x, 0, 0), (0, y, 0): area x y / 2 exactly where x y is a
    float32.  Returns (vertices, faces, the expected area_q per component)."""
    u = 2.0 ** -20
    nan, inf = float("nan"), float("inf")
    legs = [(u, u, 0),                     # 0.5 units: the half rounds down to the even 0
            (u, 3 * u, 2),                 # 1.5 -> 2, up to even
            (u, 5 * u, 2),                 # 2.5 -> 2, down to even
            (u, 7 * u, 4),                 # 3.5 -> 4
            (u, 2 * u, 1),                 # exactly 1
            (1.0, 1.0, 1 << 39),
            (2.0 ** 12, 2.0 ** 11, 1 << 62),                       # exactly the clamp
            (2.0 ** 12, 2.0 ** 11 * (1 - 2.0 ** -23), (1 << 62) - (1 << 39)),      # the float32 below it: not clamped
            (2.0 ** 13, 2.0 ** 13, 1 << 62),                       # 2^65 units, clamped
            (2.0 ** 70, 2.0 ** 70, 0),                             # the cross product overflows to an infinity: counts 0
            (nan, 1.0, 0), (1.0, inf, 0), (-inf, 1.0, 0)]
    v, want = [], []
    for x, y, q in legs:
        v += [[0, 0, 0], [x, 0, 0], [0, y, 0]]
        want.append(q)
    v += [[0, 0, 0], [1, 1, 1], [2, 2, 2]]                        # collinear: zero area
    want.append(0)
    v += [[1, 2, 3], [1, 2, 3], [4, 5, 6]]                        # two corners coincide
    want.append(0)
    v = np.array(v, np.float32)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3), want
