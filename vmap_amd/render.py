"""View rendering on the device: all object fields composited per pixel of a camera image (csrc/view_kernels.h, field_query_seg_s32
of csrc/query_split_kernels.h, field_query_seg_gen of csrc/query_kernels.h; the contract is the view section of include/vmapstep.h).

``render_view`` takes the stacked fields of one hidden width, one oriented box per object (``meshing.BoundingBox``, ``bounds.get_bounds`` -
anything with ``.center``, ``.R`` with the axes as columns, ``.extent``), a camera-to-world pose and the intrinsics, and returns depth,
colour, opacity and instance images in the width-major layout of every image here.  Per band of pixels: count the (object, pixel)
hits, read their number (the one host synchronisation), allocate the pair and sample buffers, then one call that packs the parameter
images, emits the pairs, evaluates every sample of every pair with the segmented field kernel and merges per pixel.  The pixel range is
cut into bands when the buffers of one call would exceed ``budget_bytes``; a pixel's result does not depend on the band it is in, so
the images are the same bits however the range is cut.  GPU only: there is no eager path.

``render_view_groups`` renders up to four ``FieldGroup`` s into ONE image: each group has its own hidden width (32, 64, ..., 256) and
its own samples per hit - the object stack at hidden 32 with 16 samples plus the background model at hidden 128 in its room box with
48 is the two-group case.  Objects are numbered through the groups in order (``View.instance``).  There is one path: ``render_view`` is
the one-group call of it.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _devmem, _lib
from .bounds import _intrinsics4

__all__ = ["View", "FieldGroup", "render_view", "render_view_groups", "stack_fields", "MAX_HITS", "MAX_SAMPLES", "MAX_OBJECTS", "MAX_GROUPS"]

MAX_HITS = _lib.VIEW_MAX_HITS
MAX_SAMPLES = 64
MAX_OBJECTS = 256
MAX_GROUPS = _lib.VIEW_MAX_GROUPS
WIDTHS = tuple(range(32, 257, 32))         # hidden widths a field group may have
BYTES_PER_SAMPLE = 16                      # occupancy + colour: what a band's budget is counted in
BLOCK = 64                                 # pixels per block of the geometry kernels: bands start on multiples of it


@dataclass
class View:
    depth: torch.Tensor                    # [W, H] float32
    color: torch.Tensor                    # [W, H, 3] float32
    opacity: torch.Tensor                  # [W, H] float32
    instance: torch.Tensor                 # [W, H] int32: index into the object list, -1 where no box is hit
    overflow: int                          # pixels that hit more than MAX_HITS boxes (the nearest MAX_HITS were composited)
    n_pairs: int                           # (object, pixel) hits over the rendered range
    bands: int = 1
    # return_samples (one band): the kernel's intermediate buffers
    pairs: Optional[torch.Tensor] = None       # [n_pairs, 4] int32: pixel, t_near bits, dt bits, 0 - ordered by (object, pixel)
    offsets: Optional[np.ndarray] = None       # [n_obj + 1] int64 (host)
    sample_occ: Optional[torch.Tensor] = None  # [n_pairs, S]
    sample_rgb: Optional[torch.Tensor] = None  # [n_pairs, S, 3]
    # render_view_groups with return_samples: sample_occ / sample_rgb above are the flat buffers ([n_samples], [n_samples, 3]: group
    # after group); below the split per group, each as render_view of that group alone returns it (offsets starting at 0)
    group_pairs: Optional[list] = None         # [g] -> [pairs_g, 4] int32
    group_offsets: Optional[list] = None       # [g] -> [n_obj_g + 1] int64 (host)
    group_sample_occ: Optional[list] = None    # [g] -> [pairs_g, S_g]
    group_sample_rgb: Optional[list] = None    # [g] -> [pairs_g, S_g, 3]


@dataclass
class FieldGroup:
    """Fields of ONE hidden width rendered with ``samples`` samples per hit: ``fields`` as ``render_view`` takes them, one box per
    field, the field-frame centres (default zeros)."""
    fields: object
    boxes: list
    centers: object = None
    samples: int = 16


def stack_fields(fields):
    """(fc tensors [14 x [n, ...]], pe_B [n, 21, 3], pe_scale [n]) from a ``HipMapper`` (its slab views and ``scale``: no copy), a list
    of ``Trainer`` s (their parameters stacked once) or the stacked triple itself."""
    if hasattr(fields, "trainers") and hasattr(fields, "views"):            # driver.HipMapper
        if fields.slab is not None and not fields._dirty:
            return list(fields.views[:14]), fields.views[14], fields.scale
        fields = fields.trainers
    if isinstance(fields, (tuple, list)) and len(fields) == 3 and torch.is_tensor(fields[1]):
        fc, pe_B, scale = fields
        return list(fc), pe_B, scale
    trainers = list(fields)
    if not trainers:
        raise _lib.VmapStepError("render_view: no fields")
    with torch.no_grad():
        cols = [list(tr.fc_occ_map.parameters()) for tr in trainers]
        fc = [torch.stack([c[t].detach() for c in cols]).contiguous() for t in range(_lib.NUM_FC)]
        pe_B = torch.stack([tr.pe.B_layer.weight.detach() for tr in trainers]).contiguous()
        dev = pe_B.device
        scale = torch.stack([tr.pe.scale.detach().to(dev, torch.float32).reshape(()) for tr in trainers]).contiguous()
    return fc, pe_B, scale


def _box_rows(boxes, n):
    """float32 [n, 15] (centre, row-major R, extent); ``None`` -> a box of zero extent, which no ray crosses (t_far <= t_near)."""
    if len(boxes) != n:
        raise _lib.VmapStepError(f"render_view: {len(boxes)} boxes for {n} fields")
    rows = np.zeros((n, 15), np.float32)
    for k, b in enumerate(boxes):
        if b is None:
            rows[k, 3:12] = np.eye(3, dtype=np.float32).reshape(-1)
            continue
        tonp = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        rows[k, 0:3] = tonp(b.center).astype(np.float32).reshape(3)
        rows[k, 3:12] = tonp(b.R).astype(np.float32).reshape(9)
        rows[k, 12:15] = tonp(b.extent).astype(np.float32).reshape(3)
    return rows


def render_view(fields, boxes, t_wc, intrinsics, width, height, samples=16, min_depth=0.0, centers=None, pixel_range=None,
                budget_bytes=256 << 20, return_samples=False) -> View:
    """Render the objects ``fields`` inside their ``boxes`` from the camera-to-world pose ``t_wc`` ([4, 4]): the one-group case of
    ``render_view_groups``, at every hidden width.

    ``centers``: the field-frame centre of every object ([n, 3], the objects' ``obj_center``; default zeros).  ``pixel_range``:
    (begin, end) of the pixel index w * height + h to render (default the whole image; the other pixels stay 0 / -1).
    ``budget_bytes``: the sample buffers of one call; a range that needs more is rendered in bands.  ``return_samples``: also return the
    pair records, offsets and per-sample occupancy / colour - of ONE call, so the budget is not applied: ``View.sample_occ`` is
    [n_pairs, S] and ``View.sample_rgb`` [n_pairs, S, 3], and the ``group_*`` lists hold the same one group."""
    v = _render_groups("render_view", [FieldGroup(fields, boxes, centers, samples)], t_wc, intrinsics, width, height, min_depth, pixel_range,
                       budget_bytes, return_samples)
    if v.group_pairs is not None:
        v.sample_occ, v.sample_rgb = v.group_sample_occ[0], v.group_sample_rgb[0]
    return v


def _prepare_group(name, g, dev):
    """The C view of one FieldGroup: (ViewGroup fields, box rows, centres, keep-alive objects).  ``name``: the caller, for the messages."""
    fc, pe_B, scale = stack_fields(g.fields)
    n = int(pe_B.shape[0])
    if dev is not None and pe_B.device != dev:
        raise _lib.VmapStepError(f"{name}: all groups must be on one device")
    dev = pe_B.device
    if dev.type != "cuda":
        raise _lib.VmapStepError(f"{name} runs on the GPU (no CPU fallback)")
    if len(fc) != _lib.NUM_FC or int(fc[0].shape[1]) not in WIDTHS:
        raise _lib.VmapStepError(f"{name}: hidden widths 32, 64, ..., 256 only")
    pp = _lib.Params()
    for t, p in enumerate(list(fc) + [pe_B]):
        if p.dtype != torch.float32 or p.device != dev or p.shape[0] != n or not p[0].is_contiguous():
            raise _lib.VmapStepError(f"{name}: field parameters must be float32, on one device, stacked over the objects and contiguous per object")
        ref = _lib.Tensor(p.data_ptr(), p.stride(0))
        if t < _lib.NUM_FC:
            pp.fc[t] = ref
        else:
            pp.pe_B = ref
    scale = scale.to(dev, torch.float32).reshape(n).contiguous()
    sc = _lib.Tensor(scale.data_ptr(), 1)
    rows = _box_rows(list(g.boxes), n)
    if g.centers is None:
        centers = torch.zeros(n, 3, dtype=torch.float32, device=dev)
    else:
        c = g.centers
        centers = torch.as_tensor(np.asarray([[float(v) for v in (x if x is not None else (0, 0, 0))] for x in c], np.float32)
                                  if not torch.is_tensor(c) else c).to(dev, torch.float32).reshape(n, 3).contiguous()
    return dict(hidden=int(fc[0].shape[1]), n=n, samples=int(g.samples), pp=pp, sc=sc, rows=rows, centers=centers, keep=(fc, pe_B, scale)), dev


@torch.no_grad()
def render_view_groups(groups, t_wc, intrinsics, width, height, min_depth=0.0, pixel_range=None, budget_bytes=256 << 20,
                       return_samples=False) -> View:
    """Render the ``FieldGroup`` s ``groups`` (1 .. MAX_GROUPS) into one image from the camera-to-world pose ``t_wc``: every group's
    fields are sampled inside their boxes with the group's own sample count and all samples of a pixel are merged as ``render_view``
    merges them.  ``View.instance`` numbers the objects through the groups in order.  The other arguments are ``render_view``'s; a
    band's bytes sum over the groups' own sample counts."""
    return _render_groups("render_view_groups", groups, t_wc, intrinsics, width, height, min_depth, pixel_range, budget_bytes, return_samples)


@torch.no_grad()
def _render_groups(name, groups, t_wc, intrinsics, width, height, min_depth, pixel_range, budget_bytes, return_samples):
    groups = list(groups)
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise _lib.VmapStepError(f"{name}: 1 .. {MAX_GROUPS} groups ({len(groups)} given)")
    dev, G = None, []
    for g in groups:
        d, dev = _prepare_group(name, g, dev)
        G.append(d)
    ng = len(G)
    n = sum(d["n"] for d in G)
    first = np.concatenate([[0], np.cumsum([d["n"] for d in G])]).astype(int)
    S = [d["samples"] for d in G]
    width, height = int(width), int(height)
    lib = _lib.load()
    garr = (_lib.ViewGroup * ng)(*[_lib.ViewGroup(d["hidden"], d["n"], d["samples"], 0, ctypes.pointer(d["pp"]), ctypes.pointer(d["sc"])) for d in G])
    boxes_d = torch.from_numpy(np.concatenate([d["rows"] for d in G])).to(dev)
    centers_d = torch.cat([d["centers"] for d in G]).contiguous()
    T = (t_wc.detach().cpu().numpy() if torch.is_tensor(t_wc) else np.asarray(t_wc)).astype(np.float32).reshape(4, 4)
    fx, fy, cx, cy = _intrinsics4(intrinsics)
    npix = width * height
    p0, p1 = (0, npix) if pixel_range is None else (int(pixel_range[0]), int(pixel_range[1]))

    def cfg_of(b, e):                          # samples and n_obj are not read by the scene entry points
        return _lib.ViewCfg(width, height, 0, n, fx, fy, cx, cy, (ctypes.c_float * 16)(*T.reshape(-1)), float(min_depth), b, e)

    depth = torch.zeros(width, height, dtype=torch.float32, device=dev)
    color = torch.zeros(width, height, 3, dtype=torch.float32, device=dev)
    opacity = torch.zeros(width, height, dtype=torch.float32, device=dev)
    instance = torch.full((width, height), -1, dtype=torch.int32, device=dev)
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    offsets_d = torch.empty(n + 1, dtype=torch.int64, device=dev)
    total, bands, kept = 0, 0, None

    def band(b, e):
        nonlocal total, bands, kept
        cfg = cfg_of(b, e)
        ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_scene_view_workspace_bytes, dev, ctypes.byref(cfg), garr, ng)
        _lib.check(lib.vmapstep_scene_view_count(ctypes.byref(cfg), garr, ng, boxes_d.data_ptr(), offsets_d.data_ptr(), ws_ptr, nbytes,
                                                 _devmem.stream(dev)), lib)
        off_h = offsets_d.cpu().numpy().copy()           # the one host synchronisation of the band
        m = int(off_h[-1])
        mg = [int(off_h[first[i + 1]] - off_h[first[i]]) for i in range(ng)]
        ns = sum(mg[i] * S[i] for i in range(ng))
        need = ns * BYTES_PER_SAMPLE
        if not return_samples and need > budget_bytes and e - b > BLOCK:
            parts = min(-(-need // max(int(budget_bytes), 1)), -(-(e - b) // BLOCK))
            step = -(-(e - b) // parts)
            step = -(-step // BLOCK) * BLOCK
            cuts = list(range(b, e, step)) + [e]
            if len(cuts) == 2:                           # cannot be cut on a block boundary any finer: halve
                cuts = [b, b + max(BLOCK, (e - b) // 2 // BLOCK * BLOCK), e]
            del ws
            for i in range(len(cuts) - 1):
                band(cuts[i], cuts[i + 1])
            return
        pairs = torch.empty(max(m, 1), 4, dtype=torch.int32, device=dev)
        occ = torch.empty(max(ns, 1), dtype=torch.float32, device=dev)
        rgb = torch.empty(max(ns, 1), 3, dtype=torch.float32, device=dev)
        _lib.check(lib.vmapstep_scene_view_render(ctypes.byref(cfg), garr, ng, boxes_d.data_ptr(), centers_d.data_ptr(),
                                                  offsets_d.data_ptr(), off_h.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                  pairs.data_ptr(), m, occ.data_ptr(), rgb.data_ptr(),
                                                  depth.data_ptr(), color.data_ptr(), opacity.data_ptr(), instance.data_ptr(), overflow.data_ptr(),
                                                  ws_ptr, nbytes, _devmem.stream(dev)), lib)
        total += m
        bands += 1
        if return_samples:
            kept = (pairs[:m], off_h, occ[:ns], rgb[:ns], mg)
        # offsets_d is rewritten by the next band's count: same stream, so the order holds

    with torch.cuda.device(dev):
        if p1 > p0:
            band(p0, p1)
        ovf = int(overflow.item())
    view = View(depth, color, opacity, instance, ovf, total, bands)
    if return_samples and kept is not None:
        pairs, off_h, occ, rgb, mg = kept
        view.pairs, view.offsets, view.sample_occ, view.sample_rgb = pairs, off_h, occ, rgb
        view.group_pairs, view.group_offsets, view.group_sample_occ, view.group_sample_rgb = [], [], [], []
        at = 0
        for i in range(ng):
            a = int(off_h[first[i]])
            view.group_pairs.append(pairs[a:a + mg[i]])
            view.group_offsets.append(off_h[first[i]:first[i + 1] + 1] - a)
            view.group_sample_occ.append(occ[at:at + mg[i] * S[i]].view(mg[i], S[i]))
            view.group_sample_rgb.append(rgb[at:at + mg[i] * S[i]].view(mg[i], S[i], 3))
            at += mg[i] * S[i]
    return view
