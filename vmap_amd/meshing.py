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

from . import _lib


class BoundingBox:
    """The reference's utils.BoundingBox: centre [3], rotation R [3,3] and full extent [3] of an object box.  Anything with the same
    three attributes (an open3d OrientedBoundingBox) works where a bound is expected."""

    def __init__(self, center=None, R=None, extent=None):
        self.center = np.zeros(3) if center is None else np.asarray(center, np.float64)
        self.R = np.eye(3) if R is None else np.asarray(R, np.float64)
        self.extent = np.ones(3) if extent is None else np.asarray(extent, np.float64)


class Mesh:
    """Device tensors: vertices float32 [V,3], faces int32 [F,3], vertex_normals float32 [V,3], vertex_colors uint8 [V,3] or None."""

    def __init__(self, vertices, faces, vertex_normals, vertex_colors=None):
        self.vertices = vertices
        self.faces = faces
        self.vertex_normals = vertex_normals
        self.vertex_colors = vertex_colors

    def numpy(self):
        """(vertices, faces, vertex_normals, vertex_colors or None) as host arrays."""
        c = None if self.vertex_colors is None else self.vertex_colors.cpu().numpy()
        return self.vertices.cpu().numpy(), self.faces.cpu().numpy(), self.vertex_normals.cpu().numpy(), c

    def export(self, path):
        """Write ``.obj`` (``v x y z [r g b]`` with colour in [0, 1], ``vn``, ``f a//a b//b c//c``, 1-based) or binary little-endian
        ``.ply`` (float x y z, float nx ny nz, uchar red green blue if coloured; int32 vertex indices)."""
        v, f, n, c = self.numpy()
        if str(path).lower().endswith(".obj"):
            with open(path, "w") as fh:
                if c is None:
                    fh.writelines(f"v {x:.7g} {y:.7g} {z:.7g}\n" for x, y, z in v)
                else:
                    fh.writelines(f"v {p[0]:.7g} {p[1]:.7g} {p[2]:.7g} {q[0] / 255:.6g} {q[1] / 255:.6g} {q[2] / 255:.6g}\n" for p, q in zip(v, c))
                fh.writelines(f"vn {x:.7g} {y:.7g} {z:.7g}\n" for x, y, z in n)
                fh.writelines(f"f {a}//{a} {b}//{b} {d}//{d}\n" for a, b, d in (f.astype(np.int64) + 1))
        elif str(path).lower().endswith(".ply"):
            props = ["property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz"]
            fields = [("p", "<f4", 3), ("n", "<f4", 3)]
            if c is not None:
                props += ["property uchar red", "property uchar green", "property uchar blue"]
                fields.append(("c", "u1", 3))
            head = "\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + props
                             + [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]) + "\n"
            vert = np.zeros(len(v), dtype=fields)
            vert["p"], vert["n"] = v, n
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


def _f12(affine):
    a = np.ascontiguousarray(np.asarray(affine, np.float64).reshape(3, 4), np.float32).reshape(-1)
    return (ctypes.c_float * 12)(*a.tolist())


def _workspace(shape, device):
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    _lib.check(lib.vmapstep_mesh_workspace_bytes(*shape, ctypes.byref(nb)), lib)
    ws = torch.empty(nb.value + 256, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256, nb.value


def grid_points(shape, affine, device="cuda:0"):
    """[nx*ny*nz, 3] float32 points A (i, j, k) + b in C order over the grid (one launch of vmapstep_mesh_grid_points)."""
    lib = _lib.load()
    nx, ny, nz = (int(s) for s in shape)
    dev = torch.device(device)
    pts = torch.empty(nx * ny * nz, 3, dtype=torch.float32, device=dev)
    _lib.check(lib.vmapstep_mesh_grid_points(nx, ny, nz, _f12(affine), pts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), lib)
    return pts


def extract_mesh(volume: torch.Tensor, level: float = 0.5, affine=None):
    """Marching cubes on the device over a CUDA float32 [nx, ny, nz] volume (any side >= 2).  ``affine``: optional [3,4] (rows
    [A | b]) applied to the index-space vertices, the normals mapped by A^-T.  Returns a ``Mesh`` (no colours), or ``None`` where
    the reference's vis.marching_cubes returns None: no face (which covers a level outside the volume's range)."""
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda or volume.dtype != torch.float32 or volume.dim() != 3:
        raise _lib.VmapStepError("extract_mesh: a CUDA float32 [nx, ny, nz] volume is required (no CPU fallback)")
    lib = _lib.load()
    vol = volume.contiguous()
    dev = vol.device
    shape = tuple(int(s) for s in vol.shape)
    ws, ws_ptr, nbytes = _workspace(shape, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.check(lib.vmapstep_mesh_count(vol.data_ptr(), *shape, float(level), counts.data_ptr(), ws_ptr, nbytes, stream), lib)
    nv, nf = (int(x) for x in counts.cpu())              # the one host synchronisation
    if nf == 0:
        return None
    verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    aff = None if affine is None else _f12(affine)
    _lib.check(lib.vmapstep_mesh_emit(vol.data_ptr(), *shape, float(level), aff, verts.data_ptr(), normals.data_ptr(), faces.data_ptr(),
                                      nv, nf, ws_ptr, nbytes, stream), lib)
    return Mesh(verts, faces, normals)


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

