"""Numpy checker of mesh components (vmap_amd/components.py, csrc/component_kernels.h, csrc/component_rules.h), written from the
contract of the components section of include/vmapstep.h, not from the kernels: a sequential union-find, the float32 area with every
operation rounded on its own as the header rounds it, the integer sums, the selection.  Its labels can be held against an outside
implementation - scipy.sparse.csgraph.connected_components on the edge graph (tests/test_components.py does) - the areas and the
selection are this project's own."""
from __future__ import annotations

import numpy as np

from cull_oracle import cull_faces

f32 = np.float32
AREA_CLAMP = 1 << 62


def valid_faces(faces, n_vertices):
    """bool [F]: every index of the face names a vertex."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((faces >= 0) & (faces < n_vertices)).all(1)


def label(faces, n_vertices):
    """(labels int32 [n_vertices], C): components numbered in ascending order of their smallest vertex.  A sequential union-find
    with path halving; which root wins a union does not matter here - the numbering is made from the members."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in faces[valid_faces(faces, n_vertices)].tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[rx] = ry
    root = np.array([find(v) for v in range(n_vertices)], np.int64)
    smallest = np.full(n_vertices, n_vertices, np.int64)
    np.minimum.at(smallest, root, np.arange(n_vertices))          # the smallest member of every tree, at its root
    key = smallest[root] if n_vertices else root                  # per vertex: its component's smallest vertex
    firsts = np.unique(key)
    return np.searchsorted(firsts, key).astype(np.int32), len(firsts)


def triangle_area_f32(vertices, faces):
    """float32 [F]: a = p1 - p0, b = p2 - p0, c = a x b as two rounded products and one rounded subtraction per component,
    0.5 * sqrt((c0 c0 + c1 c1) + c2 c2) - numpy rounds every float32 operation on its own and its sqrt is IEEE."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        a, b = p1 - p0, p2 - p0
        c0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        c1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        c2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        s = (c0 * c0 + c1 * c1) + c2 * c2
        area = f32(0.5) * np.sqrt(s)
    assert area.dtype == np.float32
    return area


def quantise_area(area):
    """int64 [n]: rint((double)area * 2^40) half to even; NaN, infinities, zero and negatives 0; clamped at 2^62."""
    a = np.asarray(area, np.float32).reshape(-1)
    ok = np.isfinite(a) & (a > 0)
    q = np.where(ok, a.astype(np.float64), 0.0) * 2.0 ** 40
    big = q >= 2.0 ** 62
    return np.where(big, AREA_CLAMP, np.rint(np.where(big, 0.0, q)).astype(np.int64)).astype(np.int64)


def area_threshold(min_area):
    q = float(min_area) * 2.0 ** 40
    if not q > 0:
        return 0
    return AREA_CLAMP if q >= 2.0 ** 62 else int(np.rint(q))


def stats(vertices, faces, labels, n_components):
    """(n_vertices int32 [C], n_faces int64 [C], area_q int64 [C]); vertices None: areas 0.  Integer sums (wrapping like int64)."""
    labels = np.asarray(labels, np.int64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(faces, len(labels))
    vf = faces[ok]
    comp = labels[vf[:, 0]] if len(vf) else np.zeros(0, np.int64)
    nv = np.bincount(labels, minlength=n_components).astype(np.int32)
    nf = np.bincount(comp, minlength=n_components).astype(np.int64)
    aq = np.zeros(n_components, np.uint64)
    if vertices is not None and len(vf):
        np.add.at(aq, comp, quantise_area(triangle_area_f32(vertices, vf)).astype(np.uint64))
    return nv, nf, aq.astype(np.int64)


def select(n_faces, area_q, min_faces=0, min_area=0.0, largest=None):
    """bool [C]: enough faces, enough area and - with largest = k - among the k largest by area_q, ties to the lower number."""
    n_faces, area_q = np.asarray(n_faces, np.int64), np.asarray(area_q, np.int64)
    keep = (n_faces >= min_faces) & (area_q >= area_threshold(min_area))
    if largest is not None:
        order = sorted(range(len(area_q)), key=lambda c: (-int(area_q[c]), c))
        among = np.zeros(len(area_q), bool)
        among[order[:largest]] = True
        keep &= among
    return keep


def keep_components(vertices, faces, min_faces=0, min_area=0.0, largest=None):
    """(faces_out, kept_vertices, labels, C, stats, keep): the whole path - the compaction is cull_oracle.cull_faces with min_seen 3.
    faces_out has no row when nothing is left."""
    n = len(np.asarray(vertices).reshape(-1, 3))
    labels, C = label(faces, n)
    st = stats(vertices, faces, labels, C)
    keep = select(st[1], st[2], min_faces, min_area, largest)
    mask = keep[labels] if C else np.zeros(n, bool)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    faces = faces[valid_faces(faces, n)]                          # cull_mesh drops a face with an index out of range, as every entry point does
    faces_out, kept_vertices = cull_faces(faces, mask, 3) if n else (np.zeros((0, 3), np.int32), np.zeros(0, np.int32))
    return faces_out, kept_vertices, labels, C, st, keep


def partition(labels):
    """The partition of the vertices as a set of frozensets: what must not change under a renumbering."""
    groups = {}
    for v, c in enumerate(np.asarray(labels).tolist()):
        groups.setdefault(c, []).append(v)
    return {frozenset(g) for g in groups.values()}
