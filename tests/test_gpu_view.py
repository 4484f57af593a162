"""GPU tier of the view renderer (vmap_amd/render.py; csrc/view_kernels.h, field_query_seg_s32 of csrc/query_split_kernels.h) against
tests/view_oracle.py: the pair list bit for bit against the host build of csrc/view_geometry.h, the segmented field kernel bit for bit
against Trainer.eval_points, the per-pixel merge against the checker's float64 merge of the kernel's own buffers, the cap, banding,
the existing ray forward (VmapStep.render), the whole renderer against the float64 checker, and a trained scene."""
import numpy as np
import pytest
import torch

import view_oracle as vo
from vmap_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STD = vo.Standard
U = 2.0 ** -24


class B3:
    """A box as render_view takes it."""
    def __init__(self, b):
        self.center, self.R, self.extent = b.center, b.R, b.extent


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return vo.build_host_program(tmp_path_factory.mktemp("view_host"))


def stacked(params):
    fc, B, sc = params
    return [torch.from_numpy(a).to(DEV) for a in fc], torch.from_numpy(B).to(DEV), torch.from_numpy(sc).to(DEV)


@pytest.fixture(scope="module")
def std_params():
    return synth.make_params(4, 32, seed=5)


@pytest.fixture(scope="module")
def std_view(std_params):
    """The standard scene from view 0 with the kernel's intermediate buffers: computed once, shared, never modified."""
    from vmap_amd import render
    T = vo.ring_pose(*STD.VIEWS[0])
    centers = np.array([[0.1, -0.05, 0.02], [0.0, 0.0, 0.0], [-0.03, 0.02, 0.05], [0.0, 0.1, -0.1]], np.float32)
    v = render.render_view(stacked(std_params), [B3(b) for b in STD.boxes()], T, STD.k4(), STD.W, STD.H, samples=STD.S, min_depth=STD.MIN_DEPTH,
                           centers=centers, return_samples=True)
    torch.cuda.synchronize()
    return T, centers, v


def extra_boxes(T):
    """The standard boxes + one behind the camera (an empty segment, in the middle of the list) + one around the camera."""
    pos, z = T[:3, 3].astype(np.float64), T[:3, 2].astype(np.float64)
    b = STD.boxes()
    return b[:2] + [vo.Box(pos - 2.0 * z, np.eye(3), (0.5, 0.5, 0.5))] + b[2:] + [vo.Box(pos + 0.1 * z, vo.bo.rotation((1, 1, 0), 0.4), (1.0, 1.2, 0.8))]


PAIR_CASES = {
    "96x64": lambda: (vo.ring_pose(*STD.VIEWS[0]), STD.k4(), 96, 64, None, None),
    "160x120 (1200 block totals: past the scan's first 1024-entry chunk)": lambda: (vo.ring_pose(*STD.VIEWS[1]), STD.k4(160, 120, 150.0), 160, 120, STD.boxes(), None),
    "96x64, pixels [37, 5001)": lambda: (vo.ring_pose(*STD.VIEWS[2]), STD.k4(), 96, 64, None, (37, 5001)),
    "axis-aligned pose, integer cx: exact zero direction components": lambda: (np.eye(4, dtype=np.float32), (40.0, 40.0, 16.0, 12.0), 32, 24, [
        vo.Box((0, 0, 2), np.eye(3), (1, 1, 1)), vo.Box((0, 0, 0), np.eye(3), (1, 1, 1)), vo.Box((0, 0, -3), np.eye(3), (1, 1, 1)),
        vo.Box((0.5, 0, 2), np.eye(3), (1, 2, 0.5))], (3, 700)),
}


@pytest.mark.parametrize("case", list(PAIR_CASES), ids=list(PAIR_CASES))
def test_pairs_equal_the_host_program(host_exe, tmp_path, case):
    """view_count / view_scan / view_emit: the device's offsets and pair records (pixel, t_near, dt, 0) equal, bit for bit and in
    (object, pixel) order, what the host build of the same geometry header prints - with a box behind the camera (an empty segment),
    the camera inside a box (t_near = min_depth), pixel ranges that are no multiples of 64 and rays with exact zero components."""
    from vmap_amd import render
    T, k4, W, H, boxes, rng = PAIR_CASES[case]()
    boxes = extra_boxes(T) if boxes is None else boxes
    S, md = 5, 0.05
    n = len(boxes)
    v = render.render_view(stacked(synth.make_params(n, 32, seed=2)), [B3(b) for b in boxes], T, k4, W, H, samples=S, min_depth=md, pixel_range=rng,
                           return_samples=True)
    hit, tn, dt = vo.run_host_program(host_exe, tmp_path, T, k4, W, H, boxes, S, md)
    off, px, ptn, pdt = vo.pairs_of(hit, tn, dt, *(rng or (0, W * H)))
    assert v.n_pairs == off[-1] and np.array_equal(v.offsets, off), (v.offsets, off)
    got = v.pairs.cpu().numpy()
    assert np.array_equal(got[:, 0], px) and (got[:, 3] == 0).all()
    assert np.array_equal(got[:, 1].view(np.uint32), ptn.view(np.uint32)) and np.array_equal(got[:, 2].view(np.uint32), pdt.view(np.uint32))
    if n == 6:
        assert off[3] == off[2] and off[6] - off[5] == (rng[1] - rng[0] if rng else W * H)        # behind: empty; around: every pixel
        assert (ptn[off[5]:] == np.float32(md)).all()
    # pixels outside the range are untouched
    if rng:
        inst = v.instance.reshape(-1)
        assert (inst[:rng[0]] == -1).all() and (inst[rng[1]:] == -1).all() and float(v.opacity.reshape(-1)[rng[1]:].abs().max()) == 0.0


def random_boxes(n, seed):
    rng = np.random.default_rng(seed)
    R = vo.bo.random_rotations(rng, n)
    return [vo.Box(rng.uniform(-0.9, 0.9, 3), R[k], rng.uniform(0.3, 1.2, 3)) for k in range(n)]


FIELD_CASES = [(1, 1, 24, 16), (4, 5, 96, 64), (4, 16, 96, 64), (21, 64, 24, 16)]


@pytest.mark.parametrize("n_obj,S,W,H", FIELD_CASES, ids=[f"n{c[0]}-S{c[1]}" for c in FIELD_CASES])
def test_segmented_field_kernel_equals_eval_points(n_obj, S, W, H):
    """field_query_seg_s32 against the one-object query kernel behind Trainer.eval_points, bit for bit and per object: the points are
    rebuilt from the pair records with the contract's operation order - the ray and t_s by the checker's exact float32 emulation,
    (o + d * t) - center by three separately rounded torch operations.  Segment lengths are no multiples of 128 points (asserted), rays
    straddle 32-point tiles whenever 32 % S != 0.  Premise, asserted on the inputs: every point takes the fast sine path in both
    kernels (|B x / scale| * 32 pi < 2^20)."""
    from vmap_amd import render
    from vmap_amd.trainer import SimpleConfig, Trainer
    params = synth.make_params(n_obj, 32, seed=5 + n_obj)
    fc, B, sc = params
    boxes = STD.boxes()[:n_obj] if n_obj <= 4 else random_boxes(n_obj, 1)
    centers = np.random.default_rng(7).uniform(-0.1, 0.1, (n_obj, 3)).astype(np.float32)
    T = vo.ring_pose(*STD.VIEWS[0])
    k4 = STD.k4(W, H, 90.0 * W / 96)
    v = render.render_view(stacked(params), [B3(b) for b in boxes], T, k4, W, H, samples=S, min_depth=STD.MIN_DEPTH, centers=centers, return_samples=True)
    o, d = vo.rays32(T, k4, W, H)
    pairs = v.pairs.cpu().numpy()
    tr = Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=32, obj_scale=float(sc[0])))
    seg = np.diff(v.offsets)
    assert seg.sum() == v.n_pairs > 0 and ((seg * S) % 128 != 0).any(), seg
    for k in range(n_obj):
        a, b = int(v.offsets[k]), int(v.offsets[k + 1])
        if a == b:
            continue
        with torch.no_grad():
            for p, src in zip(list(tr.fc_occ_map.parameters()) + [tr.pe.B_layer.weight], list(fc) + [B]):
                p.copy_(torch.from_numpy(src[k]))
        ts = vo.sample_depths32(pairs[a:b, 1].view(np.float32), pairs[a:b, 2].view(np.float32), S)
        dd = torch.from_numpy(d[pairs[a:b, 0]]).to(DEV)
        pts = ((torch.from_numpy(o).to(DEV)[None, None] + dd[:, None, :] * torch.from_numpy(ts).to(DEV)[:, :, None])
               - torch.from_numpy(centers[k]).to(DEV)[None, None]).reshape(-1, 3)
        proj = (pts.double().cpu().numpy() / float(sc[k])) @ B[k].astype(np.float64).T
        assert np.abs(proj).max() * 32 * np.pi < 2.0 ** 20
        occ, col = tr._eval_points_hip(pts)
        assert torch.equal(occ.view(-1, S), v.sample_occ[a:b]), k
        assert torch.equal(col.view(-1, S, 3), v.sample_rgb[a:b]), k


def merge_of(v, W, H, n, S, cap=True):
    """The checker's float64 merge of the kernel's own pair and sample buffers (sample depths by the exact float32 emulation)."""
    P = W * H
    pairs = v.pairs.cpu().numpy()
    hit = np.zeros((n, P), bool)
    t, occ, rgb, tn = np.zeros((n, P, S)), np.zeros((n, P, S)), np.zeros((n, P, S, 3)), np.full((n, P), np.inf)
    so, sr = v.sample_occ.cpu().numpy(), v.sample_rgb.cpu().numpy()
    for k in range(n):
        a, b = int(v.offsets[k]), int(v.offsets[k + 1])
        px = pairs[a:b, 0]
        hit[k, px] = True
        tn[k, px] = pairs[a:b, 1].view(np.float32)
        t[k, px] = vo.sample_depths32(pairs[a:b, 1].view(np.float32), pairs[a:b, 2].view(np.float32), S)
        occ[k, px], rgb[k, px] = so[a:b], sr[a:b]
    return vo.composite(P, hit, t, occ, rgb, t_near=tn if cap else None), t


def check_merge(v, m, t, S):
    """Bound of the device's float32 merge against the float64 one, N = hits * S terms (at most 16 S): the transmittance in front of
    term i carries 2 roundings per factor and one per product (3 (i - 1) u), w_i = occ_i T_i and w_i v_i one each, the running sum at
    most N - 1 more: every term within (3 (N - 1) + 2 + (N - 1)) u < 4 N u of its own size, so |difference| <= 4 N u sum_i w_i |v_i|
    <= 4 N u * opacity * max |v| (u = 2^-24; opacity itself: max |v| = 1)."""
    N = np.minimum(m["n_hits"], vo.MAX_HITS) * S
    tmax = np.abs(t).max(axis=(0, 2))
    for name, got, want, vmax in (("depth", v.depth, m["depth"], tmax), ("colour", v.color, m["color"], 1.0), ("opacity", v.opacity, m["opacity"], 1.0)):
        bound = 4 * N * U * m["opacity"] * vmax + 1e-30
        got = got.cpu().numpy().astype(np.float64).reshape(want.shape)
        err = np.abs(got - want)
        b = bound if err.ndim == 1 else bound[:, None]
        print(f"{name}: max |device - float64 merge| {err.max():.3e}, largest bound {bound.max():.3e}, worst ratio {np.max(err / b):.3f}")
        assert (err <= b).all(), name
    top = np.sort(m["weights"], 1)[:, -2:] if m["weights"].shape[1] > 1 else np.concatenate([np.zeros_like(m["weights"]), m["weights"]], 1)
    clear = (top[:, 1] - top[:, 0] > 1e-4) | (m["n_hits"] == 0)
    inst = v.instance.cpu().numpy().reshape(-1)
    assert np.array_equal(inst[clear], m["instance"][clear]) and clear.mean() > 0.5
    assert np.array_equal(inst == -1, m["n_hits"] == 0)


def test_composite_equals_the_float64_merge_of_its_own_buffers(std_view):
    _, _, v = std_view
    m, t = merge_of(v, STD.W, STD.H, 4, STD.S)
    assert v.overflow == 0 == m["overflow"] and m["n_hits"].max() >= 3
    check_merge(v, m, t, STD.S)


def test_more_than_sixteen_boxes_composite_the_nearest_sixteen():
    """20 thin slabs across the optical axis, listed out of depth order (so kept entries are replaced while the list is walked); the
    last six are narrow, so only the middle columns cross all 20.  overflow = the checker's count of pixels with more than 16 hits,
    and those pixels composite their 16 nearest by (t_near, k): the merge bound of check_merge holds with the cap applied."""
    from vmap_amd import render
    W, H, S, n = 24, 8, 4, 20
    k4 = (30.0, 30.0, 11.5, 3.5)
    boxes = [vo.Box((0, 0, 1.0 + 0.2 * ((7 * k) % 20)), np.eye(3), ((0.4 if k >= 14 else 8.0), 8.0, 0.05)) for k in range(n)]
    params = synth.make_params(n, 32, seed=9)
    params[0][8] *= np.float32(0.1)                 # out_alpha: thin media (occupancy around sigmoid(-3)), so that the slabs behind the
    params[0][9][:] = np.float32(-0.3)              # sixteenth still carry weight and the cap changes the image
    v = render.render_view(stacked(params), [B3(b) for b in boxes], np.eye(4, dtype=np.float32), k4, W, H, samples=S, min_depth=0.05, return_samples=True)
    m, t = merge_of(v, W, H, n, S)
    uncapped, _ = merge_of(v, W, H, n, S, cap=False)
    over = uncapped["n_hits"] > vo.MAX_HITS
    print(f"pixels with more than 16 hits: {over.sum()} of {W * H}; device overflow {v.overflow}")
    assert 0 < over.sum() < W * H and v.overflow == m["overflow"] == over.sum()
    check_merge(v, m, t, S)
    assert np.abs(uncapped["opacity"] - m["opacity"])[over].max() > 1e-3          # the cap is visible: the test can tell the two apart


def test_bands_and_repeats_are_bit_identical(std_params, std_view):
    from vmap_amd import render
    T, centers, one = std_view
    args = (stacked(std_params), [B3(b) for b in STD.boxes()], T, STD.k4(), STD.W, STD.H)
    kw = dict(samples=STD.S, min_depth=STD.MIN_DEPTH, centers=centers)
    images = lambda v: (v.depth, v.color, v.opacity, v.instance)
    again = render.render_view(*args, **kw)
    small = render.render_view(*args, budget_bytes=300_000, **kw)
    assert again.bands == 1 and small.bands > 2 and small.n_pairs == one.n_pairs == again.n_pairs
    for a, b, c in zip(images(one), images(again), images(small)):
        assert torch.equal(a, b) and torch.equal(a, c)
    P = STD.W * STD.H
    cuts = [0, 1000, 1001 + 64 * 31 + 17, P]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = render.render_view(*args, pixel_range=(lo, hi), **kw)
        for a, b in zip(images(one), images(part)):
            a, b = a.reshape(P, -1), b.reshape(P, -1)
            assert torch.equal(a[lo:hi], b[lo:hi])
            assert float(b[:lo].abs().sum() + b[hi:].abs().sum()) == (0.0 if b.dtype.is_floating_point else float(P - (hi - lo)))


def test_single_hit_pixels_equal_the_ray_forward_of_the_step(std_params, std_view):
    """The existing forward: for pixels that hit exactly one object, that object's t_s as z and the pixel's ray as a step.RayPoints
    through VmapStep.render give render_depth / render_color / opacity equal to the view's within 2e-5 relative (the figure
    tests/test_gpu_parity.py uses for render outputs)."""
    from conftest import make_op
    from vmap_amd import step
    T, centers, v = std_view
    fc, B, sc = stacked(std_params)
    pairs = v.pairs.cpu().numpy()
    counts = np.bincount(pairs[:, 0], minlength=STD.W * STD.H)
    o, d = vo.rays32(T, STD.k4(), STD.W, STD.H)
    R = 40
    sel, compared = [], []
    for k in range(4):
        a, b = int(v.offsets[k]), int(v.offsets[k + 1])
        rows = a + np.nonzero(counts[pairs[a:b, 0]] == 1)[0]
        compared.append(len(rows) >= R)                       # a box that lies wholly in front of others has no such pixel: its rays
        rows = rows if compared[-1] else np.arange(a, b)      # only fill the batch
        sel.append(rows[np.linspace(0, len(rows) - 1, R).astype(int)])
    assert sum(compared) >= 3, compared
    sel = np.stack(sel)                                                          # [4, R] pair rows
    px = pairs[sel, 0]
    z = torch.from_numpy(vo.sample_depths32(pairs[sel, 1].view(np.float32), pairs[sel, 2].view(np.float32), STD.S)).to(DEV)
    rays = step.RayPoints(torch.from_numpy(np.broadcast_to(o, (4, R, 3)).copy()).to(DEV), torch.from_numpy(d[px]).to(DEV), torch.from_numpy(centers).to(DEV))
    op = make_op(4, R, STD.S, 32, device=DEV)
    zeros = torch.zeros(4, R, device=DEV)
    res = op.render(fc, B, sc, rays, z, zeros, torch.zeros(4, R, 3, device=DEV), torch.ones(4, R, dtype=torch.uint8, device=DEV),
                    torch.ones(4, R, dtype=torch.uint8, device=DEV))
    idx = torch.from_numpy(px.astype(np.int64)).to(DEV)
    use = torch.tensor(compared, device=DEV)
    for name, got, want in (("depth", v.depth.reshape(-1)[idx], res.render_depth), ("colour", v.color.reshape(-1, 3)[idx], res.render_color),
                            ("opacity", v.opacity.reshape(-1)[idx], res.opacity)):
        got, want = got[use], want[use]
        rel = float((got - want).abs().max() / want.abs().max())
        print(f"{name}: relative difference to VmapStep.render {rel:.3e}")
        assert rel <= 2e-5, name


# twice the worst |float32-emulated geometry - float64 geometry| of the checker's own outputs over the three standard views, outside
# the edge pixels (measured on the CPU with tests/view_oracle.render_checker: depth 1.98e-5, colour 1.05e-5, opacity 5.96e-6)
GEOMETRY_TERM = {"depth": 2 * 1.98e-5, "color": 2 * 1.05e-5, "opacity": 2 * 5.96e-6}


@pytest.mark.parametrize("view", range(len(STD.VIEWS)))
def test_view_against_the_float64_checker(std_params, view):
    """End to end on the standard scene (centres zero, as in the CPU measurement).  Per pixel the limit is the sum of a field term -
    the query kernel's 2e-5 tolerance propagated to first order through the composite: (sum_i |d out / d occ_i| + sum_i w_i) * 2e-5,
    computed by the checker - and a geometry term: GEOMETRY_TERM, twice the worst difference between the checker's float32-emulated
    geometry and its float64 self on this scene (measured on the CPU over the three views: depth 1.98e-5, colour 1.05e-5, opacity
    5.96e-6; twice: the emulation's sums are not ordered as the device's).  Edge pixels (any
    object's float64 |t_far - t_near| < 1e-4) are excluded and must stay <= 1 %."""
    from vmap_amd import render
    T = vo.ring_pose(*STD.VIEWS[view])
    centers = np.zeros((4, 3), np.float32)
    v = render.render_view(stacked(std_params), [B3(b) for b in STD.boxes()], T, STD.k4(), STD.W, STD.H, samples=STD.S, min_depth=STD.MIN_DEPTH, centers=centers)
    ref = vo.render_checker(T, STD.k4(), STD.W, STD.H, STD.boxes(), centers, STD.S, STD.MIN_DEPTH, std_params, with_sensitivity=True)
    ok = ~ref["edge"]
    assert ref["edge"].mean() <= 0.01
    for key, got in (("depth", v.depth), ("color", v.color), ("opacity", v.opacity)):
        got = got.cpu().numpy().astype(np.float64).reshape(ref[key].shape)
        err = np.abs(got - ref[key])[ok]
        lim = (2e-5 * ref["sensitivity"][key] + GEOMETRY_TERM[key])[ok]
        print(f"{key}: max |device - checker| {err.max():.3e}; limit there {lim.reshape(err.shape).flat[err.argmax()]:.3e}; worst ratio {(err / lim).max():.3f}")
        assert (err <= lim).all(), key
    top = np.sort(ref["weights"], 1)[:, -2:]
    clear = ok & ((top[:, 1] - top[:, 0] > 1e-4) | (ref["n_hits"] == 0))
    assert np.array_equal(v.instance.cpu().numpy().reshape(-1)[clear], ref["instance"][clear])


# ---- a trained scene: the scaffold of tests/test_pipeline.py (same spheres, same 16 frames) -----------------------------------------

PW, PH = 96, 72
PFX = PFY = 80.0
PCX, PCY = (PW - 1) / 2.0, (PH - 1) / 2.0
SPHERES = {1: (np.array([-0.45, 0.0, 2.2], np.float32), 0.45, (220, 40, 40)),
           2: (np.array([0.55, 0.1, 2.6], np.float32), 0.40, (40, 60, 230))}
WALL_Z = 4.0


def render_frame(t_wc):
    iw, ih = np.meshgrid(np.arange(PW, dtype=np.float32), np.arange(PH, dtype=np.float32), indexing="ij")
    d_c = np.stack([(iw - PCX) / PFX, (ih - PCY) / PFY, np.ones_like(iw)], -1)
    R, o = t_wc[:3, :3], t_wc[:3, 3]
    d_w = d_c @ R.T
    depth = np.full((PW, PH), np.inf, np.float32)
    inst = np.zeros((PW, PH), np.int32)
    rgb = np.zeros((PW, PH, 3), np.uint8)
    rgb[:] = (120, 120, 120)
    tw = (WALL_Z - o[2]) / d_w[..., 2]
    depth = np.where(tw > 0, tw, depth).astype(np.float32)
    for oid, (c, r, col) in SPHERES.items():
        oc = o - c
        a = (d_w * d_w).sum(-1)
        b = 2.0 * (d_w * oc).sum(-1)
        cc = (oc * oc).sum() - r * r
        disc = b * b - 4 * a * cc
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        hit = (t > 0) & (t < depth)
        depth = np.where(hit, t, depth).astype(np.float32)
        inst = np.where(hit, oid, inst)
        rgb[hit] = col
    return rgb, depth.astype(np.float32), inst


def bbox_of(inst, oid):
    ws, hs = np.nonzero(inst == oid)
    return np.array([ws.min(), ws.max(), hs.min(), hs.max()], np.float32)


def test_trained_scene_renders_its_spheres():
    """Train the two spheres as tests/test_pipeline.py does, then HipMapper.render_view from a training pose (frame 8) with axis-aligned
    cubes of side 2 r + 0.2 around them, S = 16: over the pixels of each sphere the median |depth - analytic depth| < 0.25 (the
    pipeline test's own figure for this scene and budget) and `instance` names the sphere on more than half of them."""
    from vmap_amd import sampler
    from vmap_amd.driver import HipMapper
    from vmap_amd.keyframes import FrameStore, ObjectKeyframes
    from vmap_amd.trainer import SimpleConfig, Trainer
    torch.manual_seed(0)
    cfg = SimpleConfig(training_device=DEV, hidden_feature_size=32, n_iter_per_frame=20, n_per_optim=120, win_size=5)
    store = FrameStore(12, PW, PH, device=DEV)
    oks, trainers = {}, {}
    mapper = HipMapper(cfg, device=DEV)
    smp = sampler.FrameSampler(PW, PH, 100, 24, 1, 9, PFX, PFY, PCX, PCY, min_depth=0.0, surface_eps=0.1, stop_eps=0.05, device=DEV, seed=3)
    for fid in range(16):
        ang = 0.06 * (fid - 7.5)
        t_wc = np.eye(4, dtype=np.float32)
        t_wc[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
        t_wc[:3, 3] = [0.6 * np.sin(ang) * 2.4, 0.0, 2.4 - 2.4 * np.cos(ang)]
        rgb, depth, inst = render_frame(t_wc)
        if fid == 8:
            seen = (t_wc, depth, inst)                             # the pose the view is rendered from: both spheres in sight
        slot = store.put(torch.from_numpy(rgb), torch.from_numpy(depth), torch.from_numpy(inst), torch.from_numpy(t_wc), fid)
        for oid, (c, r, _) in SPHERES.items():
            if not (inst == oid).any():
                continue
            if oid not in oks:
                oks[oid] = ObjectKeyframes(store, oid, slot, bbox_of(inst, oid), keyframe_buffer_size=6, center=tuple(float(v) for v in c))
                trainers[oid] = Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=32, obj_scale=1.0))
                mapper.add_object(trainers[oid])
            else:
                oks[oid].append(slot, bbox_of(inst, oid))
        store.collect()
        smp.set_objects([oks[o].sampler_entry() for o in sorted(oks)])
        fr = smp.sample()
        mapper.check_flags(mapper.train_frame(fr["pcs"], fr["z"], fr["gt_depth"], fr["gt_rgb"], fr["sem"], fr["depth_mask"]))
    order = sorted(oks)                                            # add_object order: both spheres are in the first frame
    cubes = [vo.Box(SPHERES[o][0], np.eye(3), (2 * SPHERES[o][1] + 0.2,) * 3) for o in order]
    t_wc, depth, inst = seen
    view = mapper.render_view(cubes, t_wc, (PFX, PFY, PCX, PCY), PW, PH, centers=[SPHERES[o][0] for o in order], samples=16)
    got_d, got_i = view.depth.cpu().numpy(), view.instance.cpu().numpy()
    for k, oid in enumerate(order):
        on = inst == oid
        err = np.abs(got_d - depth)[on]
        named = (got_i[on] == k).mean()
        print(f"sphere {oid}: {on.sum()} pixels, median |depth - analytic| {np.median(err):.3f}, instance right on {named:.2%}")
        assert on.sum() > 100 and np.median(err) < 0.25 and named > 0.5, oid
