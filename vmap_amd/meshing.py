"""Mesh extraction on the device: marching cubes over an occupancy volume (vmapstep_mesh_count / _emit, csrc/mesh_kernels.h) and the
mesh container the reference builds with trimesh in vis.py:6-19.

``extract_mesh`` is the reference's ``vis.marching_cubes`` (skimage.measure.marching_cubes, level 0.5, gradient_direction='ascent')
without the host round trip; ``Trainer.meshing`` (trainer.py) puts the grid, the queries and the transforms around it.
Deviations from the reference, all deliberate:
- the classic (Lorensen) triangle table instead of Lewiner's: the vertices are the same, triangles differ only in cells whose classic
  configuration is ambiguous (skimage's method='lorensen' gives the same mesh up to vertex order);
- vertex normals are numpy.gradient's central differences interpolated along the edge, not skimage's own formula (they agree in
  direction on smooth fields, not on rough ones);
- ``None`` whenever no face results: a level outside [min, max] (skimage raises ValueError), and a level equal to the volume's
  maximum exactly (no corner lies strictly above it; skimage passes its range check, then raises RuntimeError for the empty
  surface, so the reference's vis.marching_cubes returns None there as well);
- ``Mesh.export`` is this module's own OBJ / PLY writer, not trimesh's.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _devmem, _lib


class BoundingBox:
    """The reference's utils.BoundingBox: centre [3], rotation R [3,3] and full extent [3] of an object box.  Anything with the same
    three attributes (an open3d OrientedBoundingBox) works where a bound is expected."""

    def __init__(self, center=None, R=None, extent=None):
        self.center = np.zeros(3) if center is None else np.asarray(center, np.float64)
        self.R = np.eye(3) if R is None else np.asarray(R, np.float64)
        self.extent = np.ones(3) if extent is None else np.asarray(extent, np.float64)


class Mesh:
    """Device tensors: vertices float32 [V,3], faces int32 [F,3], vertex_normals float32 [V,3] or None, vertex_colors uint8 [V,3]
    or None."""

    def __init__(self, vertices, faces, vertex_normals, vertex_colors=None):
        self.vertices = vertices
        self.faces = faces
        self.vertex_normals = vertex_normals
        self.vertex_colors = vertex_colors

    def numpy(self):
        """(vertices, faces, vertex_normals or None, vertex_colors or None) as host arrays."""
        c = None if self.vertex_colors is None else self.vertex_colors.cpu().numpy()
        n = None if self.vertex_normals is None else self.vertex_normals.cpu().numpy()
        return self.vertices.cpu().numpy(), self.faces.cpu().numpy(), n, c

    def export(self, path):
        """Write ``.obj`` (``v x y z [r g b]`` with colour in [0, 1], ``vn``, ``f a//a b//b c//c``, 1-based) or binary little-endian
        ``.ply`` (float x y z, float nx ny nz, uchar red green blue if coloured; int32 vertex indices).  Without normals: no ``vn``
        lines and ``f a b c`` (OBJ), no normal properties (PLY)."""
        v, f, n, c = self.numpy()
        if str(path).lower().endswith(".obj"):
            with open(path, "w") as fh:
                if c is None:
                    fh.writelines(f"v {x:.7g} {y:.7g} {z:.7g}\n" for x, y, z in v)
                else:
                    fh.writelines(f"v {p[0]:.7g} {p[1]:.7g} {p[2]:.7g} {q[0] / 255:.6g} {q[1] / 255:.6g} {q[2] / 255:.6g}\n" for p, q in zip(v, c))
                if n is None:
                    fh.writelines(f"f {a} {b} {d}\n" for a, b, d in (f.astype(np.int64) + 1))
                else:
                    fh.writelines(f"vn {x:.7g} {y:.7g} {z:.7g}\n" for x, y, z in n)
                    fh.writelines(f"f {a}//{a} {b}//{b} {d}//{d}\n" for a, b, d in (f.astype(np.int64) + 1))
        elif str(path).lower().endswith(".ply"):
            props = ["property float x", "property float y", "property float z"]
            fields = [("p", "<f4", 3)]
            if n is not None:
                props += ["property float nx", "property float ny", "property float nz"]
                fields.append(("n", "<f4", 3))
            if c is not None:
                props += ["property uchar red", "property uchar green", "property uchar blue"]
                fields.append(("c", "u1", 3))
            head = "\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + props
                             + [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]) + "\n"
            vert = np.zeros(len(v), dtype=fields)
            vert["p"] = v
            if n is not None:
                vert["n"] = n
            if c is not None:
                vert["c"] = c
            face = np.zeros(len(f), dtype=[("k", "u1"), ("i", "<i4", 3)])
            face["k"], face["i"] = 3, f
            with open(path, "wb") as fh:
                fh.write(head.encode("ascii"))
                fh.write(vert.tobytes())
                fh.write(face.tobytes())
        else:
            raise ValueError(f"{path}: export writes .obj or .ply")


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _fan(polys):
    """Triangles (a, b_k, b_{k+1}) from polygons given as lists of vertex indices (k-gons with k >= 3; shorter ones dropped)."""
    tris = [(p[0], p[k], p[k + 1]) for p in polys for k in range(1, len(p) - 1)]
    return np.asarray(tris, np.int64).reshape(-1, 3)


def _read_obj(path):
    verts, polys = [], []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                verts.append([float(x) for x in t[1:4]])
            elif t[0] == "f":
                idx = [int(x.split("/")[0]) for x in t[1:]]
                polys.append([i - 1 if i > 0 else len(verts) + i for i in idx])      # 1-based; negative = relative
    return np.asarray(verts, np.float64).reshape(-1, 3), _fan(polys)


def _read_ply(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:body].decode("ascii", "replace").splitlines():
        t = line.split()
        if not t:
            continue
        if t[0] == "format":
            fmt = t[1]
        elif t[0] == "element":
            elements.append((t[1], int(t[2]), []))
        elif t[0] == "property":
            if t[1] == "list":
                elements[-1][2].append((t[4], ("list", _PLY_TYPES[t[2]], _PLY_TYPES[t[3]])))
            else:
                elements[-1][2].append((t[2], _PLY_TYPES[t[1]]))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r}")
    verts, polys = None, []
    if fmt == "ascii":
        words = data[body:].split()
        pos = 0
        for name, count, props in elements:
            rows = []
            for _ in range(count):
                row = {}
                for pname, ptype in props:
                    if isinstance(ptype, tuple):
                        k = int(words[pos])
                        row[pname] = [int(float(w)) for w in words[pos + 1:pos + 1 + k]]
                        pos += 1 + k
                    else:
                        row[pname] = float(words[pos])
                        pos += 1
                rows.append(row)
            if name == "vertex":
                verts = np.asarray([[r["x"], r["y"], r["z"]] for r in rows], np.float64).reshape(-1, 3)
            elif name == "face":
                key = "vertex_indices" if any(p == "vertex_indices" for p, _ in props) else "vertex_index"
                polys = [r[key] for r in rows]
    else:
        e = "<" if fmt == "binary_little_endian" else ">"
        pos = body
        for name, count, props in elements:
            if not any(isinstance(t, tuple) for _, t in props):
                dt = np.dtype([(pn, e + pt) for pn, pt in props])
                arr = np.frombuffer(data, dt, count, pos)
                pos += dt.itemsize * count
                if name == "vertex":
                    verts = np.stack([arr["x"], arr["y"], arr["z"]], 1).astype(np.float64)
                continue
            rows = []
            for _ in range(count):           # elements with a list property: one record at a time
                row = {}
                for pname, ptype in props:
                    if isinstance(ptype, tuple):
                        ct, it = np.dtype(e + ptype[1]), np.dtype(e + ptype[2])
                        k = int(np.frombuffer(data, ct, 1, pos)[0])
                        pos += ct.itemsize
                        row[pname] = np.frombuffer(data, it, k, pos).astype(np.int64).tolist()
                        pos += it.itemsize * k
                    else:
                        pos += np.dtype(ptype).itemsize
                rows.append(row)
            if name == "face":
                key = "vertex_indices" if any(p == "vertex_indices" for p, _ in props) else "vertex_index"
                polys = [r[key] for r in rows]
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    return verts, _fan(polys)


def load_mesh(path, device="cuda:0"):
    """Read an ``.obj`` (``v`` and ``f`` lines; ``f`` entries as a, a/t, a//n or a/t/n, negative indices relative) or ``.ply``
    (ascii or binary, any scalar property types, float or double x y z, extra vertex / face properties ignored, face lists with any
    count and index types) into a device ``Mesh`` (float32 vertices, int32 faces, no normals or colours).  Polygons with more than
    three vertices are fan-triangulated from their first vertex."""
    p = str(path).lower()
    if p.endswith(".obj"):
        v, f = _read_obj(path)
    elif p.endswith(".ply"):
        v, f = _read_ply(path)
    else:
        raise ValueError(f"{path}: load_mesh reads .obj or .ply")
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{path}: face index outside the {len(v)} vertices")
    dev = torch.device(device)
    return Mesh(torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev),
                torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev), None)


def _f12(affine):
    a = np.ascontiguousarray(np.asarray(affine, np.float64).reshape(3, 4), np.float32).reshape(-1)
    return (ctypes.c_float * 12)(*a.tolist())


def grid_points(shape, affine, device="cuda:0"):
    """[nx*ny*nz, 3] float32 points A (i, j, k) + b in C order over the grid (one launch of vmapstep_mesh_grid_points)."""
    lib = _lib.load()
    nx, ny, nz = (int(s) for s in shape)
    dev = torch.device(device)
    pts = torch.empty(nx * ny * nz, 3, dtype=torch.float32, device=dev)
    _lib.check(lib.vmapstep_mesh_grid_points(nx, ny, nz, _f12(affine), pts.data_ptr(), _devmem.stream(dev)), lib)
    return pts


def extract_mesh(volume: torch.Tensor, level: float = 0.5, affine=None, valid=None, return_edges=False):
    """Marching cubes on the device over a CUDA float32 [nx, ny, nz] volume (any side >= 2).  ``affine``: optional [3,4] (rows
    [A | b]) applied to the index-space vertices, the normals mapped by A^-T.  Returns a ``Mesh`` (no colours), or ``None`` where
    the reference's vis.marching_cubes returns None: no face (which covers a level outside the volume's range).

    ``valid``: optional mask of the volume's shape (non-zero = the point holds a value).  Only cells whose eight corners are all valid
    exist, a vertex is emitted only on an edge of an existing cell, and the normals treat an invalid neighbour like the grid border
    (the contract of vmapstep_mesh_count_valid); all ones gives the unmasked mesh bit for bit.  ``return_edges``: return
    ``(mesh, edge_ids)`` with the int32 [V] tensor owning point * 3 + axis of every vertex (``(None, None)`` without a face)."""
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda or volume.dtype != torch.float32 or volume.dim() != 3:
        raise _lib.VmapStepError("extract_mesh: a CUDA float32 [nx, ny, nz] volume is required (no CPU fallback)")
    lib = _lib.load()
    vol = volume.contiguous()
    dev = vol.device
    shape = tuple(int(s) for s in vol.shape)
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_mesh_workspace_bytes, dev, *shape)
    stream = _devmem.stream(dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    mask = None
    if valid is not None:
        mask = torch.as_tensor(valid).to(dev)
        if tuple(mask.shape) != shape:
            raise _lib.VmapStepError("extract_mesh: valid must have the volume's shape")
        mask = (mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)).contiguous()
    mask_ptr = None if mask is None else mask.data_ptr()
    _lib.check(lib.vmapstep_mesh_count_valid(vol.data_ptr(), mask_ptr, *shape, float(level), counts.data_ptr(), ws_ptr, nbytes, stream), lib)
    nv, nf = (int(x) for x in counts.cpu())              # the one host synchronisation
    if nf == 0:
        return (None, None) if return_edges else None
    verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    aff = None if affine is None else _f12(affine)
    edges = torch.empty(nv, dtype=torch.int32, device=dev) if return_edges else None
    _lib.check(lib.vmapstep_mesh_emit_valid(vol.data_ptr(), mask_ptr, *shape, float(level), aff, verts.data_ptr(), normals.data_ptr(),
                                            faces.data_ptr(), None if edges is None else edges.data_ptr(), nv, nf, ws_ptr, nbytes, stream), lib)
    mesh = Mesh(verts, faces, normals)
    return (mesh, edges) if return_edges else mesh


def bound_affine(bound, bound_extent, grid_dim, obj_center=None):
    """[3,4] float64: grid index (i, j, k) of a grid_dim^3 grid -> the reference's point (trainer.py:35-50, render_rays.py:98-122):
    t = linspace(-1, 1, D) per axis, times the scale extent / (2 bound_extent), rotated by R, shifted by the centre, minus obj_center.
    The same map takes index-space vertices to scene coordinates (trainer.py:59-64) when obj_center is None."""
    s = np.asarray(bound.extent, np.float64) / (2.0 * bound_extent)
    R = np.asarray(bound.R, np.float64)
    c = np.asarray(bound.center, np.float64).reshape(3)
    A = R * (2.0 * s / (grid_dim - 1))[None, :]
    b = c - R @ s
    if obj_center is not None:
        b = b - np.broadcast_to(np.asarray(torch.as_tensor(obj_center).detach().cpu().numpy(), np.float64), (3,))
    return np.concatenate([A, b[:, None]], 1)

