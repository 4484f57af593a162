"""Mesh components on the device: label, measure and drop floaters.

A field queried over its whole box yields the object's surface plus floaters: small closed blobs where the occupancy crosses 0.5 in
space nobody constrained.  Every sample drawn on one is far from the ground truth, so evaluation removes them first.
``label_components`` numbers the connected components of an indexed triangle mesh, ``component_stats`` counts their vertices and
faces and sums their area, ``keep_components`` drops what is too small (or all but the largest ``k``), and ``weld_vertices`` turns
separate triangles back into an indexed mesh.  The rules are csrc/component_rules.h's, the kernels csrc/component_kernels.h's, the
contract the components section of include/vmapstep.h.

Connectivity is VERTEX connectivity by shared indices: two vertices are connected iff a chain of faces links them, and sharing one
vertex is enough.  That is what ``scipy.sparse.csgraph.connected_components`` gives on the edge graph, labels included (components
are numbered in ascending order of their smallest vertex).  It is coarser than trimesh's ``split``, which goes by edge adjacency:
two sheets that touch in a single vertex are one component here and two there.  Position plays no part: a mesh of separate triangles
(``evaluation.crop_to_box``, an unindexed file) is one component per triangle until ``weld_vertices`` has merged equal positions.

Areas are integers: a triangle's float32 area in units of 2^-40 m^2, summed in int64.  The sum is exact and independent of order, so
a keep / drop decision is the same from run to run, which a float sum by atomics would not give.  There is no CPU fallback."""
from __future__ import annotations

import torch

from . import _devmem, _lib
from .meshing import Mesh

__all__ = ["ComponentStats", "label_components", "component_stats", "select_components", "keep_components", "weld_vertices", "area_threshold"]

AREA_UNIT = 2.0 ** -40                     # m^2 per unit of area_q
_AREA_CLAMP = 1 << 62


def _device():
    if not torch.cuda.is_available():
        raise _lib.VmapStepError("mesh components run on the GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def area_threshold(min_area):
    """``min_area`` (m^2) in units of 2^-40 m^2: rint(min_area * 2^40), half to even, clamped to [0, 2^62] (kr::area_threshold)."""
    a = float(min_area)
    if a != a or a < 0.0:
        raise _lib.VmapStepError("min_area must be a number >= 0")
    q = a * 2.0 ** 40
    return _AREA_CLAMP if q >= 2.0 ** 62 else int(round(q))        # round(): half to even on a float


class ComponentStats:
    """Per component, device tensors [C]: ``vertices`` (int32), ``faces`` (int64), ``area_q`` (int64, units of 2^-40 m^2);
    ``area``: float64 m^2.  ``kept``: bool [C] where a selection was made (``keep_components``), else ``None``."""

    def __init__(self, vertices, faces, area_q, kept=None):
        self.vertices = vertices
        self.faces = faces
        self.area_q = area_q
        self.kept = kept

    @property
    def area(self):
        return self.area_q.double() * AREA_UNIT

    def __len__(self):
        return int(self.vertices.numel())


def _arrays(mesh, dev):
    v = torch.as_tensor(mesh.vertices).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    f = torch.as_tensor(mesh.faces).to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    return v, f


def label_components(mesh):
    """(labels, n_components): ``labels`` int32 [V] on the device, components numbered 0 .. C - 1 in ascending order of their
    smallest vertex index.  A face with an index outside [0, V) is ignored whole; a vertex no valid face references is a component
    of its own.  One host synchronisation, for C."""
    lib = _lib.load()
    dev = _device()
    v, f = _arrays(mesh, dev)
    labels = torch.empty(len(v), dtype=torch.int32, device=dev)
    counts = torch.empty(1, dtype=torch.int64, device=dev)
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_components_workspace_bytes, dev, len(v), len(f))
    _lib.check(lib.vmapstep_components_label(f.data_ptr(), len(f), len(v), labels.data_ptr(), counts.data_ptr(), ws_ptr, nbytes,
                                             _devmem.stream(dev)), lib)
    n = int(counts.cpu())                  # the one host synchronisation
    del ws
    return labels, n


def component_stats(mesh, labels, n_components, areas=True):
    """``ComponentStats`` of ``mesh`` under ``labels`` (``label_components``'s pair).  ``areas=False`` leaves ``area_q`` 0 and reads
    no vertex."""
    lib = _lib.load()
    dev = _device()
    v, f = _arrays(mesh, dev)
    lab = torch.as_tensor(labels).to(device=dev, dtype=torch.int32).contiguous()
    C = int(n_components)
    if lab.numel() != len(v):
        raise _lib.VmapStepError("component_stats: one label per vertex")
    if not 0 <= C <= len(v):
        raise _lib.VmapStepError(f"component_stats: n_components={C} outside [0, {len(v)}]")
    nv = torch.empty(C, dtype=torch.int32, device=dev)
    nf = torch.empty(C, dtype=torch.int64, device=dev)
    aq = torch.empty(C, dtype=torch.int64, device=dev)
    _lib.check(lib.vmapstep_components_stats(v.data_ptr() if areas else None, f.data_ptr(), len(f), lab.data_ptr(), len(v), C,
                                             nv.data_ptr(), nf.data_ptr(), aq.data_ptr(), _devmem.stream(dev)), lib)
    return ComponentStats(nv, nf, aq)


def select_components(stats, min_faces=0, min_area=0.0, largest=None):
    """bool [C] on the statistics' device: the contract's selection.  A component is kept iff ``faces >= min_faces``, ``area_q >=
    area_threshold(min_area)`` and, where ``largest`` = k is given, it is among the k largest by ``area_q``, ties to the lower
    component number."""
    if int(min_faces) < 0:
        raise _lib.VmapStepError("min_faces must be >= 0")
    if largest is not None and int(largest) < 0:
        raise _lib.VmapStepError("largest must be >= 0")
    keep = (stats.faces >= int(min_faces)) & (stats.area_q >= area_threshold(min_area))
    if largest is not None:
        order = torch.sort(stats.area_q, descending=True, stable=True).indices      # stable: equal areas stay in ascending number
        among = torch.zeros_like(keep)
        among[order[:int(largest)]] = True
        keep &= among
    return keep


def keep_components(mesh, min_faces=0, min_area=0.0, largest=None, return_stats=False):
    """``mesh`` without the components the selection drops (``select_components``), as a ``Mesh``, or ``None`` when no face is left.
    A vertex is kept iff its component is; the mesh is then compacted by ``visibility.cull_mesh(mesh, keep, min_seen=3)``: faces and
    vertices keep their order, normals and colours travel with their vertices, and a vertex without a face goes.
    ``return_stats=True``: (mesh or None, the ``ComponentStats`` of the INPUT with ``kept`` set)."""
    from . import visibility
    area_threshold(min_area)               # refuses a bad threshold before any launch
    labels, C = label_components(mesh)
    stats = component_stats(mesh, labels, C)
    stats.kept = select_components(stats, min_faces, min_area, largest)
    out = None
    if C > 0:
        mask = stats.kept[labels.long()].to(torch.uint8)
        out = visibility.cull_mesh(mesh, mask, min_seen=3)
    return (out, stats) if return_stats else out


def weld_vertices(mesh):
    """``mesh`` with the vertices of equal position merged: two vertices are one iff their three float32 coordinates have equal
    bit patterns, -0.0 taken as +0.0 (so a NaN merges only with the same NaN).  The survivors are the first occurrences in their
    order, so an indexed mesh comes back unchanged and the call is idempotent; normals and colours are the first occurrence's.  A
    face with an index out of range stays out of range (all three indices -1).  torch's unique on the device: not a hot path."""
    dev = _device()
    v, f = _arrays(mesh, dev)
    n = len(v)
    if n == 0:
        return Mesh(v, f, getattr(mesh, "vertex_normals", None), getattr(mesh, "vertex_colors", None))
    bits = v.view(torch.int32)
    bits = torch.where(bits == -(1 << 31), torch.zeros_like(bits), bits)
    _, inverse = torch.unique(bits, dim=0, return_inverse=True)
    groups = int(inverse.max()) + 1
    index = torch.arange(n, device=dev)
    first = torch.full((groups,), n, dtype=torch.int64, device=dev).scatter_reduce(0, inverse, index, "amin")
    survivors = torch.sort(first).values                   # first occurrences, ascending
    rank = torch.empty(groups, dtype=torch.int64, device=dev)
    rank[torch.argsort(first)] = torch.arange(groups, device=dev)
    new = rank[inverse].to(torch.int32)                    # the new index of every old vertex
    valid = ((f >= 0) & (f < n)).all(1, keepdim=True)
    faces = torch.where(valid, new[f.clamp(0, n - 1).long()], torch.full_like(f, -1))
    gather = lambda t: None if t is None else torch.as_tensor(t).to(dev)[survivors]
    return Mesh(v[survivors], faces, gather(getattr(mesh, "vertex_normals", None)), gather(getattr(mesh, "vertex_colors", None)))
