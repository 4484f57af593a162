"""GPU tier of the scene view (vmap_amd/render.render_view_groups; the scene forms of csrc/view_kernels.h, field_query_seg_gen of
csrc/query_kernels.h) against tests/scene_view_oracle.py: field groups of their own hidden width and samples per hit in one image.
One group against render_view, the wide segmented field kernel bit for bit against Trainer.eval_points, the independence of groups,
the pair list against the host build of csrc/view_geometry.h, the merge, the cap, banding, the existing ray forward at hidden 128, the
whole renderer against the float64 checker, and HipMapper with its background model."""
import numpy as np
import pytest
import torch

import scene_view_oracle as so
import view_oracle as vo
from test_gpu_view import B3, stacked
from vmap_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STD = vo.Standard
U = 2.0 ** -24
CENTERS32 = np.array([[0.1, -0.05, 0.02], [0.0, 0.0, 0.0], [-0.03, 0.02, 0.05], [0.0, 0.1, -0.1]], np.float32)
ROOM_CENTER = np.array([[0.05, -0.1, 0.2]], np.float32)
images = lambda v: (v.depth, v.color, v.opacity, v.instance)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return vo.build_host_program(tmp_path_factory.mktemp("scene_view_host"))


@pytest.fixture(scope="module")
def params32():
    return synth.make_params(4, 32, seed=5)


@pytest.fixture(scope="module")
def params128():
    return synth.make_params(1, 128, seed=6)


def group_of(params, boxes, centers, S):
    from vmap_amd import render
    return render.FieldGroup(stacked(params), [B3(b) for b in boxes], centers, S)


def render_groups(groups, T, **kw):
    from vmap_amd import render
    kw.setdefault("min_depth", STD.MIN_DEPTH)
    return render.render_view_groups(groups, T, STD.k4(), STD.W, STD.H, **kw)


@pytest.fixture(scope="module")
def mixed(params32, params128):
    """The standard mixed scene from view 0, S = (16, 48), with the kernels' intermediate buffers: computed once, shared, never modified."""
    T = vo.ring_pose(*STD.VIEWS[0])
    groups = [group_of(params32, STD.boxes(), CENTERS32, 16), group_of(params128, [so.ROOM], ROOM_CENTER, 48)]
    v = render_groups(groups, T, return_samples=True)
    torch.cuda.synchronize()
    return T, groups, v


def test_one_hidden32_group_equals_render_view(params32):
    from vmap_amd import render
    T = vo.ring_pose(*STD.VIEWS[0])
    r = render.render_view(stacked(params32), [B3(b) for b in STD.boxes()], T, STD.k4(), STD.W, STD.H, samples=STD.S, min_depth=STD.MIN_DEPTH,
                           centers=CENTERS32, return_samples=True)
    v = render_groups([group_of(params32, STD.boxes(), CENTERS32, STD.S)], T, return_samples=True)
    assert v.n_pairs == r.n_pairs > 0 and v.overflow == r.overflow
    for a, b in zip(images(v), images(r)):
        assert torch.equal(a, b)
    assert torch.equal(v.pairs, r.pairs) and np.array_equal(v.offsets, r.offsets) and np.array_equal(v.group_offsets[0], r.offsets)
    assert torch.equal(v.group_sample_occ[0], r.sample_occ) and torch.equal(v.group_sample_rgb[0], r.sample_rgb)
    assert torch.equal(v.sample_occ.view(-1, STD.S), r.sample_occ) and torch.equal(v.sample_rgb.view(-1, STD.S, 3), r.sample_rgb)


WIDE_CASES = [(H, S, 96, 64, 2, (37, 5001)) for H in (64, 128, 160, 256) for S in (1, 7, 48)] + [(H, 1, 24, 16, 1, (5, 380)) for H in (64, 160)]


@pytest.mark.parametrize("H,S,W,Hh,n_obj,rng", WIDE_CASES, ids=[f"h{c[0]}-S{c[1]}-{c[2]}x{c[3]}" for c in WIDE_CASES])
def test_wide_segmented_field_kernel_equals_eval_points(H, S, W, Hh, n_obj, rng):
    """field_query_seg_gen<H / 32> against the one-object query kernel behind Trainer.eval_points (field_query_gen<H / 32>), bit for
    bit and per object, as test_segmented_field_kernel_equals_eval_points does at hidden 32: the points are rebuilt from the pair
    records with the contract's operation order.  A wide group of two objects (the room box, which every pixel hits, and a standard box),
    a pixel range that is no multiple of 64; hidden 160 is the first width whose second activation set lives in LDS.  Premise, asserted
    on the inputs: every point takes the fast sine path in both kernels (|B x / scale| * 32 pi < 2^20)."""
    from vmap_amd import render
    from vmap_amd.trainer import SimpleConfig, Trainer
    params = synth.make_params(n_obj, H, seed=20 + H // 32)
    fc, B, sc = params
    boxes = [so.ROOM, STD.boxes()[1]][:n_obj]
    centers = np.random.default_rng(7).uniform(-0.1, 0.1, (n_obj, 3)).astype(np.float32)
    T = vo.ring_pose(*STD.VIEWS[0])
    k4 = STD.k4(W, Hh, 90.0 * W / 96)
    v = render.render_view(stacked(params), [B3(b) for b in boxes], T, k4, W, Hh, samples=S, min_depth=STD.MIN_DEPTH, centers=centers,
                           pixel_range=rng, return_samples=True)
    o, d = vo.rays32(T, k4, W, Hh)
    pairs = v.pairs.cpu().numpy()
    tr = Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=H, obj_scale=float(sc[0])))
    seg = np.diff(v.offsets)
    assert seg.sum() == v.n_pairs > 0 and seg[0] == rng[1] - rng[0] and (seg > 0).all(), seg
    if W == 96:
        assert ((seg * S) % 128 != 0).any(), seg
    assert v.sample_occ.shape == (v.n_pairs, S) and v.sample_rgb.shape == (v.n_pairs, S, 3)
    for k in range(n_obj):
        a, b = int(v.offsets[k]), int(v.offsets[k + 1])
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


def test_a_groups_pairs_and_samples_do_not_depend_on_the_other_groups(params32, params128, mixed):
    from vmap_amd import render
    T, groups, v = mixed
    alone = [render.render_view(stacked(params32), [B3(b) for b in STD.boxes()], T, STD.k4(), STD.W, STD.H, samples=16, min_depth=STD.MIN_DEPTH,
                                centers=CENTERS32, return_samples=True),
             render.render_view(stacked(params128), [B3(so.ROOM)], T, STD.k4(), STD.W, STD.H, samples=48, min_depth=STD.MIN_DEPTH,
                                centers=ROOM_CENTER, return_samples=True)]
    assert v.n_pairs == alone[0].n_pairs + alone[1].n_pairs and alone[1].n_pairs == STD.W * STD.H
    for g, r in enumerate(alone):
        assert np.array_equal(v.group_offsets[g], r.offsets), g
        assert torch.equal(v.group_pairs[g], r.pairs), g
        assert torch.equal(v.group_sample_occ[g], r.sample_occ) and torch.equal(v.group_sample_rgb[g], r.sample_rgb), g


def test_mixed_pairs_equal_the_host_program(host_exe, tmp_path, params32):
    """The pair records of a mixed scene with S = (5, 7) equal, bit for bit and in (global object, pixel) order, what the host build of
    csrc/view_geometry.h prints with each group's S (one run per S, that group's rows taken): a box behind the camera in the middle of
    the wide group (an empty segment), a pixel range that is no multiple of 64."""
    T = vo.ring_pose(*STD.VIEWS[2])
    pos, z = T[:3, 3].astype(np.float64), T[:3, 2].astype(np.float64)
    wide = [so.ROOM, vo.Box(pos - 2.0 * z, np.eye(3), (0.5, 0.5, 0.5)), STD.boxes()[1]]
    rng = (37, 5001)
    groups = [group_of(params32, STD.boxes(), None, 5), group_of(synth.make_params(3, 64, seed=3), wide, None, 7)]
    v = render_groups(groups, T, pixel_range=rng, return_samples=True)
    boxes = STD.boxes() + wide
    rows = []
    for S, sl in ((5, slice(0, 4)), (7, slice(4, 7))):
        hit, tn, dt = vo.run_host_program(host_exe, tmp_path, T, STD.k4(), STD.W, STD.H, boxes, S, STD.MIN_DEPTH)
        rows.append((hit[sl], tn[sl], dt[sl]))
    hit, tn, dt = (np.concatenate([r[i] for r in rows]) for i in range(3))
    off, px, ptn, pdt = vo.pairs_of(hit, tn, dt, *rng)
    assert v.n_pairs == off[-1] and np.array_equal(v.offsets, off), (v.offsets, off)
    got = v.pairs.cpu().numpy()
    assert np.array_equal(got[:, 0], px) and (got[:, 3] == 0).all()
    assert np.array_equal(got[:, 1].view(np.uint32), ptn.view(np.uint32)) and np.array_equal(got[:, 2].view(np.uint32), pdt.view(np.uint32))
    assert off[6] == off[5] and off[5] - off[4] == rng[1] - rng[0]                 # behind: empty; the room: every pixel
    assert v.sample_occ.shape[0] == 5 * off[4] + 7 * (off[7] - off[4])
    inst = v.instance.reshape(-1)
    assert (inst[:rng[0]] == -1).all() and (inst[rng[1]:] == -1).all() and (inst[rng[0]:rng[1]] >= 0).all()


def merge_of(v, W, H, S_obj, cap=True):
    """The checker's float64 merge of the kernels' own pair and sample buffers (sample depths by the exact float32 emulation)."""
    P, n = W * H, len(S_obj)
    pairs = v.pairs.cpu().numpy()
    first = np.concatenate([[0], np.cumsum([len(o) - 1 for o in v.group_offsets])])
    hit = np.zeros((n, P), bool)
    tn = np.full((n, P), np.inf)
    t, occ, rgb = [], [], []
    for g in range(len(v.group_offsets)):
        so_, sr_ = v.group_sample_occ[g].cpu().numpy(), v.group_sample_rgb[g].cpu().numpy()
        base = int(v.offsets[first[g]])
        for j in range(len(v.group_offsets[g]) - 1):
            k = first[g] + j
            S = int(S_obj[k])
            a, b = int(v.offsets[k]), int(v.offsets[k + 1])
            px = pairs[a:b, 0]
            tk, ok, ck = np.zeros((P, S)), np.zeros((P, S)), np.zeros((P, S, 3))
            hit[k, px] = True
            tn[k, px] = pairs[a:b, 1].view(np.float32)
            tk[px] = vo.sample_depths32(pairs[a:b, 1].view(np.float32), pairs[a:b, 2].view(np.float32), S)
            ok[px], ck[px] = so_[a - base:b - base], sr_[a - base:b - base]
            t.append(tk); occ.append(ok); rgb.append(ck)
    return so.composite(P, hit, t, occ, rgb, S_obj, t_near=tn if cap else None), np.array([np.abs(x).max(1) for x in t]).max(0)


def check_merge(v, m, tmax):
    """test_gpu_view.check_merge with the N of a pixel generalised from hits * S to the sum of its composited entries' own sample
    counts (m["n_terms"]), derived the same way: the transmittance in front of term i carries 2 roundings per factor and one per
    product (3 (i - 1) u), w_i = occ_i T_i and w_i v_i one each, the running sum at most N - 1 more: every term within
    (3 (N - 1) + 2 + (N - 1)) u < 4 N u of its own size, so |difference| <= 4 N u * opacity * max |v|."""
    N = m["n_terms"]
    for name, got, want, vmax in (("depth", v.depth, m["depth"], tmax), ("colour", v.color, m["color"], 1.0), ("opacity", v.opacity, m["opacity"], 1.0)):
        bound = 4 * N * U * m["opacity"] * vmax + 1e-30
        got = got.cpu().numpy().astype(np.float64).reshape(want.shape)
        err = np.abs(got - want)
        b = bound if err.ndim == 1 else bound[:, None]
        print(f"{name}: max |device - float64 merge| {err.max():.3e}, largest bound {bound.max():.3e}, worst ratio {np.max(err / b):.3f}")
        assert (err <= b).all(), name
    top = np.sort(m["weights"], 1)[:, -2:]
    clear = (top[:, 1] - top[:, 0] > 1e-4) | (m["n_hits"] == 0)
    inst = v.instance.cpu().numpy().reshape(-1)
    assert np.array_equal(inst[clear], m["instance"][clear]) and clear.mean() > 0.5
    assert np.array_equal(inst == -1, m["n_hits"] == 0)


def test_mixed_composite_equals_the_float64_merge_of_its_own_buffers(mixed):
    _, _, v = mixed
    S_obj = np.array([16] * 4 + [48])
    m, tmax = merge_of(v, STD.W, STD.H, S_obj)
    assert v.overflow == 0 == m["overflow"] and m["n_hits"].max() >= 4 and m["n_hits"].min() >= 1
    assert m["n_terms"].max() >= 3 * 16 + 48
    check_merge(v, m, tmax)


def test_the_cap_with_mixed_sample_counts():
    """The 20 slabs of test_more_than_sixteen_boxes_composite_the_nearest_sixteen, alternating between a hidden-32 group (S = 4) and a
    hidden-64 group (S = 6): overflow = the checker's count, the capped pixels composite their 16 nearest by (t_near, global k)."""
    from vmap_amd import render
    W, H, n = 24, 8, 20
    k4 = (30.0, 30.0, 11.5, 3.5)
    slabs = [vo.Box((0, 0, 1.0 + 0.2 * ((7 * k) % 20)), np.eye(3), ((0.4 if k >= 14 else 8.0), 8.0, 0.05)) for k in range(n)]
    groups = []
    for g, (hidden, S) in enumerate(((32, 4), (64, 6))):
        params = synth.make_params(10, hidden, seed=9 + g)
        params[0][8] *= np.float32(0.1)                 # out_alpha: thin media, so that the slabs behind the sixteenth still carry weight
        params[0][9][:] = np.float32(-0.3)
        groups.append(group_of(params, slabs[g::2], None, S))
    v = render.render_view_groups(groups, np.eye(4, dtype=np.float32), k4, W, H, min_depth=0.05, return_samples=True)
    S_obj = np.array([4] * 10 + [6] * 10)
    m, tmax = merge_of(v, W, H, S_obj)
    uncapped, _ = merge_of(v, W, H, S_obj, cap=False)
    over = uncapped["n_hits"] > vo.MAX_HITS
    print(f"pixels with more than 16 hits: {over.sum()} of {W * H}; device overflow {v.overflow}")
    assert 0 < over.sum() < W * H and v.overflow == m["overflow"] == over.sum()
    check_merge(v, m, tmax)
    assert np.abs(uncapped["opacity"] - m["opacity"])[over].max() > 1e-3          # the cap is visible


def test_mixed_bands_ranges_and_repeats_are_bit_identical(mixed):
    T, groups, one = mixed
    again = render_groups(groups, T)
    small = render_groups(groups, T, budget_bytes=1_500_000)
    assert again.bands == 1 and small.bands > 2 and small.n_pairs == one.n_pairs == again.n_pairs
    for a, b, c in zip(images(one), images(again), images(small)):
        assert torch.equal(a, b) and torch.equal(a, c)
    P = STD.W * STD.H
    cuts = [0, 1000, 1001 + 64 * 31 + 17, P]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = render_groups(groups, T, pixel_range=(lo, hi))
        for a, b in zip(images(one), images(part)):
            a, b = a.reshape(P, -1), b.reshape(P, -1)
            assert torch.equal(a[lo:hi], b[lo:hi])
            assert float(b[:lo].abs().sum() + b[hi:].abs().sum()) == (0.0 if b.dtype.is_floating_point else float(P - (hi - lo)))


def test_room_only_pixels_equal_the_ray_forward_of_the_step(params32, params128):
    """Pixels that hit the room box alone, against VmapStep.render at hidden 128 (one object, 40 rays, the pixels' t_s as z): within
    2e-5 relative, the figure tests/test_gpu_parity.py uses for render outputs."""
    from conftest import make_op
    from vmap_amd import step
    S, R = 16, 40
    T = vo.ring_pose(*STD.VIEWS[0])
    v = render_groups([group_of(params32, STD.boxes(), CENTERS32, 16), group_of(params128, [so.ROOM], ROOM_CENTER, S)], T, return_samples=True)
    fc, B, sc = stacked(params128)
    pairs = v.pairs.cpu().numpy()
    counts = np.bincount(pairs[:, 0], minlength=STD.W * STD.H)
    a, b = int(v.offsets[4]), int(v.offsets[5])
    rows = a + np.nonzero(counts[pairs[a:b, 0]] == 1)[0]
    assert len(rows) >= R
    sel = rows[np.linspace(0, len(rows) - 1, R).astype(int)][None]               # [1, R] pair rows
    px = pairs[sel, 0]
    o, d = vo.rays32(T, STD.k4(), STD.W, STD.H)
    z = torch.from_numpy(vo.sample_depths32(pairs[sel, 1].view(np.float32), pairs[sel, 2].view(np.float32), S)).to(DEV)
    rays = step.RayPoints(torch.from_numpy(np.broadcast_to(o, (1, R, 3)).copy()).to(DEV), torch.from_numpy(d[px]).to(DEV), torch.from_numpy(ROOM_CENTER).to(DEV))
    op = make_op(1, R, S, 128, device=DEV)
    res = op.render(fc, B, sc, rays, z, torch.zeros(1, R, device=DEV), torch.zeros(1, R, 3, device=DEV), torch.ones(1, R, dtype=torch.uint8, device=DEV),
                    torch.ones(1, R, dtype=torch.uint8, device=DEV))
    idx = torch.from_numpy(px.astype(np.int64)).to(DEV)
    assert (v.instance.reshape(-1)[idx] == 4).all()
    for name, got, want in (("depth", v.depth.reshape(-1)[idx], res.render_depth), ("colour", v.color.reshape(-1, 3)[idx], res.render_color),
                            ("opacity", v.opacity.reshape(-1)[idx], res.opacity)):
        rel = float((got - want).abs().max() / want.abs().max())
        print(f"{name}: relative difference to VmapStep.render {rel:.3e}")
        assert rel <= 2e-5, name


# The mixed scene of the end-to-end test: Standard.boxes() at hidden 32 with S = 5, the room at hidden 128 with S = 7, centres zero.
# GEOMETRY_TERM: twice the worst |float32-emulated geometry - float64 geometry| of the checker's own outputs on THIS scene over the
# three standard views, outside the edge pixels, measured on the CPU with scene_view_oracle.render_checker (geometry="float32" against
# "float64"; per view: depth 1.61e-6 / 1.13e-7 / 1.32e-6, colour 1.22e-6 / 8.28e-7 / 9.04e-7, opacity 2.85e-13 / 4.4e-16 / 1.1e-14 -
# the random-init room field is opaque within its first samples, so a shifted sample barely moves the opacity; edge pixels 0 %, 0.016 %,
# 0 %).  Small sample counts keep the float64 checker (its sensitivity loop is quadratic in the samples of a pixel) at seconds.
E2E_S = (5, 7)
MEASURED = {"depth": 1.62e-6, "color": 1.22e-6, "opacity": 2.85e-13}
GEOMETRY_TERM = {k: 2 * x for k, x in MEASURED.items()}


@pytest.mark.parametrize("view", range(len(STD.VIEWS)))
def test_mixed_view_against_the_float64_checker(params32, params128, view):
    """End to end on the mixed scene.  Per pixel the limit is the sum of a field term - the query kernels' 2e-5 tolerance propagated to
    first order through the composite: (sum_i |d out / d occ_i| + sum_i w_i) * 2e-5, computed by the checker - and a geometry term:
    GEOMETRY_TERM above (twice the measured difference: the emulation's sums are not ordered as the device's).  Edge pixels (any
    object's float64 |t_far - t_near| < 1e-4) are excluded and must stay <= 1 %."""
    T = vo.ring_pose(*STD.VIEWS[view])
    v = render_groups([group_of(params32, STD.boxes(), None, E2E_S[0]), group_of(params128, [so.ROOM], None, E2E_S[1])], T)
    ref = so.render_checker(T, STD.k4(), STD.W, STD.H, [so.Group(STD.boxes(), E2E_S[0], params32), so.Group([so.ROOM], E2E_S[1], params128)],
                            STD.MIN_DEPTH, with_sensitivity=True)
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


def test_hipmapper_renders_its_background_as_the_last_group():
    """HipMapper.render_view(background_box=room) with an attached, untrained background equals render_view_groups of the object stack
    and the background's one-object stack, bit for bit; the background's instance index is the number of objects and names every pixel
    that crosses no object box; without an attached background the call raises."""
    from vmap_amd import render
    from vmap_amd.driver import HipMapper
    from vmap_amd.trainer import SimpleConfig, Trainer
    torch.manual_seed(4)
    cfg = SimpleConfig(training_device=DEV, hidden_feature_size=32)
    mapper = HipMapper(cfg, device=DEV)
    boxes = [B3(b) for b in STD.boxes()[:3]]
    for _ in boxes:
        mapper.add_object(Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=32, obj_scale=2.0)))
    T = vo.ring_pose(*STD.VIEWS[1])
    args = (T, STD.k4(), STD.W, STD.H)
    with pytest.raises(RuntimeError, match="attach_background"):
        mapper.render_view(boxes, *args, background_box=B3(so.ROOM))
    bg = Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=128, obj_scale=5.0))
    mapper.attach_background(bg, 40, 14)
    centers = [CENTERS32[k] for k in range(3)]
    v = mapper.render_view(boxes, *args, centers=centers, samples=8, min_depth=STD.MIN_DEPTH, background_box=B3(so.ROOM), background_samples=24,
                           background_center=ROOM_CENTER[0])
    want = render.render_view_groups([render.FieldGroup(mapper.trainers, boxes, centers, 8), render.FieldGroup([bg], [B3(so.ROOM)], ROOM_CENTER, 24)],
                                     *args, min_depth=STD.MIN_DEPTH)
    for a, b in zip(images(v), images(want)):
        assert torch.equal(a, b)
    objects_only = mapper.render_view(boxes, *args, centers=centers, samples=8, min_depth=STD.MIN_DEPTH)
    none = objects_only.instance == -1
    assert 0 < int(none.sum()) < none.numel() and (v.instance[none] == 3).all() and (v.instance >= 0).all()
    assert float(v.opacity[none].min()) > 0.0
