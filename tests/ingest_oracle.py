"""Numpy checker of frame ingest (vmap_amd/ingest.py, csrc/ingest_kernels.h, csrc/ingest_rules.h), written from the contract of the
ingest section of include/vmapstep.h - one full-frame mask per id, as the reference's loader works - not from the kernels.  The
fixtures tests/golden/ingest_*.npz (the reference's own output) pin it; it is the only checker for what the reference cannot
produce: MIXED, ZERO_MARGIN, overflow, id -1 and the ScanNet-style mode.

Frames come in as the image files hold them, [H, W]; everything that comes out is in [W, H] terms (u = column, v = row)."""
from __future__ import annotations

import numpy as np

ABSENT, KEPT, BACKGROUND, SMALL, ZERO_MARGIN, MIXED = range(6)


def margin(bbox_scale, extent):
    """trunc(float32(0.5 * bbox_scale) * float32(extent)): enlarge_bbox on 0-dim int64 tensors, which torch computes in float32."""
    return int(np.float32(0.5 * bbox_scale) * np.float32(extent))


def decide(idv, stats, W, H, bbox_scale=0.2, min_box=10, background=()):
    """(status, box, class) of one id from stats = (count, u_min, u_max, v_min, v_max, class_min, class_max), extremes inclusive."""
    count, u_min, u_max, v_min, v_max, c_min, c_max = (int(x) for x in stats)
    status, box, cls = ABSENT, [0, 0, 0, 0], 0
    if count > 0:
        u0, u1, v0, v1 = u_min, u_max + 1, v_min, v_max + 1
        cls = c_min
        mu, mv = margin(bbox_scale, u1 - u0), margin(bbox_scale, v1 - v0)
        if c_min != c_max:
            status = MIXED
        elif c_min in [int(b) for b in background]:
            status = BACKGROUND
        elif u1 - u0 <= min_box or v1 - v0 <= min_box:
            status = SMALL
        elif mu == 0 or mv == 0:
            status = ZERO_MARGIN
        else:
            status = KEPT
            box = [int(np.clip(u0 - mu, 0, W - 1)), int(np.clip(u1 + mu, 0, W - 1)), int(np.clip(v0 - mv, 0, H - 1)), int(np.clip(v1 + mv, 0, H - 1))]
    if idv == 0:
        box = [0, W, 0, H]
    return status, box, cls


def stats_table(inst, sem, max_ids=1024):
    """{id: (count, u_min, u_max, v_min, v_max, class_min, class_max)} over the ids in [-1, max_ids - 2], and the overflow count;
    inst, sem [H, W] (sem None: class 0)."""
    inst = np.asarray(inst).astype(np.int64)
    sem = np.zeros_like(inst) if sem is None else np.asarray(sem).astype(np.int64)
    table, overflow = {}, 0
    for i in np.unique(inst):
        m = inst == i
        if not -1 <= i <= max_ids - 2:
            overflow += int(m.sum())
            continue
        v, u = np.nonzero(m)
        c = sem[m]
        table[int(i)] = (int(m.sum()), int(u.min()), int(u.max()), int(v.min()), int(v.max()), int(c.min()), int(c.max()))
    return table, overflow


def depth_of(depth, depth_scale, max_depth):
    d = np.asarray(depth).astype(np.float32) * np.float32(depth_scale)
    d[d > np.float32(max_depth)] = 0.0
    return d


def ingest(rgb, depth, inst, sem, depth_scale, max_depth, background=(), bbox_scale=0.2, min_box=10, max_ids=1024):
    """The whole contract.  Returns a dict: rows int32 [n, 8] (id, status, count, box[4], class; ascending id, id 0 always there),
    overflow, rgbx uint8 [W, H, 4], depth float32 [W, H], inst int32 [W, H]."""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    rgbx = np.zeros((W, H, 4), np.uint8)
    rgbx[..., :3] = rgb.transpose(1, 0, 2)
    out = {"rgbx": rgbx, "depth": np.ascontiguousarray(depth_of(depth, depth_scale, max_depth).T)}
    if inst is None:
        assert sem is None
        inst_in = np.zeros((H, W), np.int64)
    else:
        inst_in = np.asarray(inst).astype(np.int64)
    table, overflow = stats_table(inst_in, sem, max_ids)
    table.setdefault(0, (0, 0, 0, 0, 0, 0, 0))
    rows, kept = [], []
    for i in sorted(table):
        status, box, cls = decide(i, table[i], W, H, bbox_scale, min_box, background)
        rows.append([i, status, table[i][0]] + box + [cls])
        if status == KEPT:
            kept.append(i)
    relabelled = np.where(np.isin(inst_in, kept), inst_in, 0).astype(np.int32)
    if inst is None:
        relabelled[:] = 0
    out.update(rows=np.asarray(rows, np.int32).reshape(-1, 8), overflow=overflow, inst=np.ascontiguousarray(relabelled.T))
    return out


def bbox_dict(rows):
    """The reference's bbox_dict from the rows: {id: [u low, u high, v low, v high]} for id 0 and every KEPT id."""
    return {int(r[0]): [int(x) for x in r[3:7]] for r in rows if r[1] == KEPT or r[0] == 0}
