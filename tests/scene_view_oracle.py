"""Checker of the scene view (vmap_amd/render.render_view_groups; the scene paragraph of the view section of include/vmapstep.h): field
groups with their own hidden width and samples per hit, all composited into one image.  Built on tests/view_oracle.py: the geometry is
view_oracle's per group (geometry32 / geometry64 with the group's sample count), the merge is view_oracle.composite with every object's
samples padded to the largest count by t = inf, occupancy 0 - composite sorts those last and ignores them.
Independent of the package: nothing here imports vmap_amd."""
import numpy as np

import view_oracle as vo

f32, f64 = np.float32, np.float64
STD = vo.Standard

# the standard mixed scene: Standard.boxes() as a hidden-32 group + one hidden-128 field in a room box around the camera ring
ROOM = vo.Box((0.2, -0.1, 0.3), vo.bo.rotation((0, 0, 1), 0.2), (8.0, 7.5, 7.0))


class Group:
    """One field group as the checker sees it: boxes, samples per hit, field-frame centres, (fc, B, scale) numpy parameters."""
    def __init__(self, boxes, S, params=None, centers=None):
        self.boxes, self.S, self.params = list(boxes), int(S), params
        self.centers = np.zeros((len(self.boxes), 3), f32) if centers is None else np.asarray(centers, f32)

    @property
    def n(self):
        return len(self.boxes)


def object_samples(groups):
    """S of every object, in the global order."""
    return np.concatenate([np.full(g.n, g.S, np.int64) for g in groups])


def geometry32(T, k4, W, H, groups, min_depth):
    """hit [n, P], t_near, dt float32 [n, P] over all groups: view_oracle.geometry32 per group with the group's S."""
    parts = [vo.geometry32(T, k4, W, H, g.boxes, g.S, min_depth) for g in groups]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def geometry64(T, k4, W, H, groups, min_depth):
    """hit, t_near, t_far, dt [n, P] over all groups and the rays: view_oracle.geometry64 per group."""
    parts = [vo.geometry64(T, k4, W, H, g.boxes, g.S, min_depth) for g in groups]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4)) + (parts[0][4],)


def pad(arrays, S_obj, fill):
    """Per-object arrays [P, S_k, ...] -> one array [n, P, S_max, ...], the tail of every object filled with ``fill``."""
    smax = int(max(S_obj))
    first = np.asarray(arrays[0])
    out = np.full((len(arrays), first.shape[0], smax) + first.shape[2:], fill, f64)
    for k, a in enumerate(arrays):
        out[k, :, :int(S_obj[k])] = a
    return out


def composite(n_pix, hit, t, occ, rgb, S_obj, t_near=None, with_sensitivity=False):
    """The contract's merge with a sample count per object.  t, occ, rgb: lists over the objects of [P, S_k], [P, S_k], [P, S_k, 3].
    view_oracle.composite on the padded arrays (t = inf, occ = 0 beyond an object's own samples); adds ``n_terms`` [P]: the samples
    of the entries composited (after the cap) - the N of the merge bound."""
    tt, oc, co = pad(t, S_obj, np.inf), pad(occ, S_obj, 0.0), pad(rgb, S_obj, 0.0)
    out = vo.composite(n_pix, hit, tt, oc, co, t_near=t_near, with_sensitivity=with_sensitivity)
    kept = np.array(hit, bool)
    if t_near is not None:
        for p in np.nonzero(kept.sum(0) > vo.MAX_HITS)[0]:
            ks = np.nonzero(kept[:, p])[0]
            order = sorted(ks, key=lambda k: (float(t_near[k, p]), int(k)))
            kept[order[vo.MAX_HITS:], p] = False
    out["n_terms"] = (kept * np.asarray(S_obj)[:, None]).sum(0)
    return out


def render_checker(T, k4, W, H, groups, min_depth, geometry="float64", with_sensitivity=False):
    """view_oracle.render_checker for field groups: geometry per group in float64 or by the float32 emulation, every group's field
    (its own parameters) and the merge in float64."""
    P = W * H
    S_obj = object_samples(groups)
    hit64, tn64, tf64, dt64, (o64, d64) = geometry64(T, k4, W, H, groups, min_depth)
    if geometry == "float32":
        hit, tn, dt = geometry32(T, k4, W, H, groups, min_depth)
        o, d = vo.rays32(T, k4, W, H)
    else:
        hit, tn, dt, o, d = hit64, tn64, dt64, o64, d64
    t, occ, rgb = [], [], []
    k = 0
    for g in groups:
        fc, B, scale = g.params
        for j in range(g.n):
            S = g.S
            tk, ok, ck = np.zeros((P, S)), np.zeros((P, S)), np.zeros((P, S, 3))
            idx = np.nonzero(hit[k])[0]
            if len(idx):
                if geometry == "float32":
                    ts = vo.sample_depths32(tn[k, idx], dt[k, idx], S)
                    pts = vo.points32(o, d[idx], ts, g.centers[j])
                else:
                    ts = tn[k, idx, None] + (np.arange(S) + 0.5)[None] * dt[k, idx, None]
                    pts = (o[None, None] + d[idx, None, :] * ts[..., None]) - np.asarray(f32(g.centers[j]), f64)[None, None]
                oc, co = vo.field64(fc, B, scale, j, pts.reshape(-1, 3))
                tk[idx], ok[idx], ck[idx] = ts, oc.reshape(-1, S), co.reshape(-1, S, 3)
            t.append(tk); occ.append(ok); rgb.append(ck)
            k += 1
    out = composite(P, hit, t, occ, rgb, S_obj, t_near=np.where(hit, tn, np.inf), with_sensitivity=with_sensitivity)
    out["hit"], out["edge"] = hit, vo.edge_pixels(tn64, tf64)
    return out
