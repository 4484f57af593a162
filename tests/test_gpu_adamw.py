"""GPU tier (`-m gpu`): the fused AdamW of every finalize form against torch.optim.AdamW's update evaluated in float64 ON GIVEN
GRADIENTS, element by element, within float32 rounding bounds (tests/adamw_ref.py).

``VmapStep.adamw_apply`` runs the finalize kernels' AdamW and image rewrite on a gradient slab the caller supplies (one row per
object: the ordered sum degenerates to a copy), so parameters, moments, gradients, step count and hyper-parameters are all free
inputs and no forward / backward noise stands between the kernel and the reference.  The tables the finalize kernels index (flat
parameter -> image position) are written by the step's prep kernel: every case calls ``prepare_frame`` first, as every caller of
``adamw_apply`` does.
"""
import numpy as np
import pytest
import torch

import adamw_ref as ar
import cases
from conftest import make_op
from oracle import vmap_oracle as vo
from vmap_amd import _lib, layout, step, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R, S = 12, 10            # the batch behind prepare_frame: the shape of cases.build_case("tiny")

# the finalize forms, as selected through the operator's tuning: (hidden, tuning, kernel family the plan must name)
ROUTES = {
    "s32": (32, None, "step_main_s32"),                                                              # step_finalize_s32
    "h32": (32, {"kernel": _lib.KERNEL_H32_F32}, "step_main_h32"),                                   # step_finalize_h32
    "h32_generic": (32, {"kernel": _lib.KERNEL_H32_F32, "generic_finalize": 1}, "step_main_h32"),    # step_finalize
    "gen96": (96, None, "step_main_gen"),                                                            # step_finalize, general layout
    "wp64": (64, None, "step_main_wp<2>"),                      # step_finalize_ws: one thread per quad from nine objects on
    "wp64_grouped": (64, {"generic_finalize": 1}, "step_main_wp<2>"),                                # step_finalize_ws, grouped
    "wp64_forced": (64, {"kernel": _lib.KERNEL_WP}, "step_main_wp<2>"),
    "ws128": (128, None, "step_main_ws<4>"),
    "ws256": (256, None, "step_main_ws<8>"),
}


def _one_thread_per_quad(route, n):
    """The launcher's rule for step_finalize_ws (csrc/ws_launch.h) on the one gradient row per object of adamw_apply: one thread per
    quad when nothing forces the grouped form and the launch has at least 512 blocks of 128 quads."""
    H, tuning, _ = ROUTES[route]
    PP = (layout.param_count(H) + 63) // 64 * 64
    return H >= 64 and H != 96 and not (tuning or {}).get("generic_finalize") and n * ((PP // 4 + 127) // 128) >= 512


class _Fixture:
    """An operator on one route with prepared tables and image, its parameters (fifteen separate tensors, or views of one
    [n, P + 7] slab - an object stride that keeps no quad 16-byte aligned), an optimiser state with given moments and step."""

    def __init__(self, route, n, weights="f32", slab=False, hyper="default", step0=0, params=None, batch=None, seed=0):
        H, tuning, kernel = ROUTES[route]
        self.route, self.n, self.H = route, n, H
        self.P = layout.param_count(H)
        self.op = make_op(n, R, S, H, device=DEV, max_steps=1, weights=weights, tuning=tuning)
        plan = self.op.plan()
        assert plan["kernel"] == kernel, (route, plan)              # a tuning that silently fell back would test another form
        hp = ar.HYPER[hyper]
        self.hp = hp
        self.opt = step.FusedAdamWState(n, H, DEV, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"])
        self.PP = self.opt.padded
        assert self.PP % 64 == 0 and self.PP - self.P >= 1
        if params is None:
            params = synth.make_params(n, H, seed=500 + seed)
        fc0, B0, sc0 = params
        self.sc = torch.from_numpy(sc0).to(DEV)
        shapes = list(layout.fc_shapes(H)) + [layout.PE_B_SHAPE]
        offs = layout.flat_offsets(H)
        self.slab = None
        if slab:
            self.slab = torch.full((n, self.P + 7), -3.0, device=DEV)
            views = [self.slab[:, offs[t]:offs[t] + layout.numel(shp)].view((n,) + tuple(shp)) for t, shp in enumerate(shapes)]
            for v, a in zip(views, list(fc0) + [B0]):
                v.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
        else:
            views = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in list(fc0) + [B0]]
        self.fc, self.B = views[:14], views[14]
        b = batch if batch is not None else synth.make_batch(n, R, S, seed=600 + seed)
        self.batch = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
        bt = self.batch
        # the prep kernel: the parameter image and the tables step_finalize_h32 / _s32 / _ws find an element's image position in
        self.op.prepare_frame(self.fc, self.B, bt["pcs"], bt["z"], bt["gt_depth"], bt["gt_rgb"], bt["sem"], bt["depth_mask"], n_steps=1)
        self.opt.step = step0
        self.pad_m = self.pad_v = None

    def args(self):
        bt = self.batch
        return (bt["pcs"], bt["z"], bt["gt_depth"], bt["gt_rgb"], bt["sem"], bt["depth_mask"])

    def params(self):
        """the parameters in flat order, float32 [n, P]"""
        return torch.cat([t.reshape(self.n, -1) for t in self.fc + [self.B]], dim=1).cpu().numpy()

    def set_params(self, p):
        o = 0
        for t in self.fc + [self.B]:
            sz = t[0].numel()
            t.copy_(torch.from_numpy(np.ascontiguousarray(p[:, o:o + sz])).to(DEV).view(t.shape))
            o += sz
        bt = self.batch       # the image follows the parameters
        self.op.prepare_frame(self.fc, self.B, bt["pcs"], bt["z"], bt["gt_depth"], bt["gt_rgb"], bt["sem"], bt["depth_mask"], n_steps=1)

    def set_moments(self, m, v):
        """m, v float32 [n, P]; the padding columns get a finite pattern no update produces"""
        n, P, PP = self.n, self.P, self.PP
        pad = np.arange(PP - P, dtype=np.float32)[None, :] + 100.0 * np.arange(n, dtype=np.float32)[:, None]
        self.pad_m, self.pad_v = (-7.25 - pad).astype(np.float32), (3.5 + pad).astype(np.float32)
        self.opt.exp_avg.copy_(torch.from_numpy(np.concatenate([m, self.pad_m], axis=1)).to(DEV))
        self.opt.exp_avg_sq.copy_(torch.from_numpy(np.concatenate([v, self.pad_v], axis=1)).to(DEV))

    def moments(self):
        return self.opt.exp_avg.cpu().numpy(), self.opt.exp_avg_sq.cpu().numpy()

    def apply(self, g):
        """one adamw_apply on gradients g [n, P]; the padding columns of the slab hold NaN (never to be read into a result)"""
        gs = np.full((self.n, self.PP), np.nan, np.float32)
        gs[:, :self.P] = g
        self.op.adamw_apply(self.fc, self.B, torch.from_numpy(gs).to(DEV), self.opt)
        torch.cuda.synchronize()

    def assert_untouched(self):
        m, v = self.moments()
        assert np.array_equal(m[:, self.P:].view(np.uint32), self.pad_m.view(np.uint32)), "padding columns of exp_avg written"
        assert np.array_equal(v[:, self.P:].view(np.uint32), self.pad_v.view(np.uint32)), "padding columns of exp_avg_sq written"
        if self.slab is not None:
            assert bool((self.slab[:, self.P:] == -3.0).all()), "slab columns behind the parameters written"


def _assert_within(got, ref, tol, what, P, mask=None):
    use = ar.bound_use(got, ref, tol)
    if mask is not None:
        use = np.where(mask, use, 0.0)
    bad = ~(use <= 1.0)                              # NaN counts as outside
    if bad.any():
        i = int(np.flatnonzero(bad.ravel())[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside their rounding bound, first [{i // P}, {i % P}]: got "
                             f"{np.asarray(got).ravel()[i]!r}, float64 {ref.ravel()[i]!r}, bound {tol.ravel()[i]:.3g} ({use.ravel()[i]:.3g} of it used)")
    return float(use.max())


def _ulps(a, b):
    """largest distance in float32 units in the last place between two finite arrays"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


def _f32_emulation(p, g, m, v, step_after, hp):
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in (hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"]))
    with np.errstate(all="ignore"):
        return vo.adamw_update(p, g, m, v, step_after, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, dtype=np.float32)


# (route, objects, weights, storage as slab views, start step, hyper-parameters): not the full product - every route sees every
# start step and every hyper-parameter set, both weight modes and both storage forms; nine objects (the XCD-affine block map of
# step_finalize_ws with blocks that exit early; hidden 64: its one-thread-per-quad form) on every route but the largest slab once
def _matrix():
    steps, hypers, rows = (0, 999, 20000), ("default", "fast", "slow"), []
    for i, route in enumerate(ROUTES):
        st = [steps[(i + k) % 3] for k in range(3)]
        hy = [hypers[(i + k) % 3] for k in range(3)]
        rows += [(route, 3, "f32", False, st[0], hy[0]), (route, 9, "bf16", True, st[1], hy[2]),
                 (route, 3 if route == "ws256" else 9, "f32", True, st[2], hy[1]), (route, 3, "bf16", False, st[1], hy[0])]
    return rows


MATRIX = _matrix()


@pytest.mark.parametrize("route,n,weights,slab,step0,hyper", MATRIX)
def test_adamw_apply_matches_float64_update(route, n, weights, slab, step0, hyper):
    """Three consecutive updates with fresh gradients over fifteen decades, from non-zero moments at an early, a late and a very late
    step: before each call the device's own p, m, v are read back and the reference is applied to THOSE, so the one-step bound holds
    without accumulated drift.  Every element of p, m, v within its bound; padding untouched; nothing non-finite; the step advances.
    And the same bits as the float32 op-by-op evaluation of the update (oracle.vmap_oracle.adamw_update)."""
    seed = list(ROUTES).index(route) * 8 + (step0 % 7)
    fx = _Fixture(route, n, weights, slab, hyper, step0, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    P = fx.P
    p0, g, m0, v0 = ar.make_inputs(rng, (n, P))
    fx.set_params(p0)
    fx.set_moments(m0, v0)
    hp = fx.hp
    worst_ulps = [0, 0, 0]
    for call in range(3):
        p0 = fx.params()
        m0, v0 = (a[:, :P] for a in fx.moments())
        if call:
            g = ar.make_gradients(rng, (n, P))
        fx.apply(g)
        assert fx.opt.step == step0 + call + 1
        p1, (m1, v1) = fx.params(), fx.moments()
        rp, rm, rv, tol_p, tol_m, tol_v = ar.adamw_f64(p0, g, m0, v0, step0 + call + 1, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
        what = f"{route} n={n} {weights} slab={slab} step {step0 + call + 1} {hyper}"
        use = [_assert_within(m1[:, :P], rm, tol_m, what + ": exp_avg", P), _assert_within(v1[:, :P], rv, tol_v, what + ": exp_avg_sq", P),
               _assert_within(p1, rp, tol_p, what + ": parameters", P)]
        assert np.isfinite(p1).all()
        fx.assert_untouched()
        ep, em, ev = _f32_emulation(p0, g, m0, v0, step0 + call + 1, hp)
        worst_ulps = [max(w, _ulps(a, b)) for w, a, b in zip(worst_ulps, (p1, m1[:, :P], v1[:, :P]), (ep, em, ev))]
    print(f"{what}: last call used {use[2]:.2f} / {use[0]:.2f} / {use[1]:.2f} of tol_p / tol_m / tol_v; "
          f"distance from the float32 op-by-op emulation: {worst_ulps[0]} / {worst_ulps[1]} / {worst_ulps[2]} ulp (p / m / v)")
    # Measured on the MI355X: 0 ulp on every route - the device build's sqrtf and / are correctly rounded and nothing is contracted
    # into a fused multiply-add, so the kernels ARE the op-by-op float32 evaluation.  Held, on top of the float64 bound: a build
    # flag or a rewrite of adamw_elem that changes a rounding shows here first.
    assert worst_ulps == [0, 0, 0], f"{what}: p / m / v are {worst_ulps} ulp from the float32 op-by-op evaluation"


def _one_update(route, n, weights, slab, seed, hyper, step0):
    fx = _Fixture(route, n, weights, slab, hyper, step0, seed=seed)
    rng = np.random.default_rng(seed)
    p0, g, m0, v0 = ar.make_inputs(rng, (n, fx.P))
    fx.set_params(p0)
    fx.set_moments(m0, v0)
    fx.apply(g)
    m, v = fx.moments()
    fx.assert_untouched()
    return fx.params(), m, v


@pytest.mark.parametrize("routes,weights,slab,hyper", [(("s32", "h32", "h32_generic"), "f32", False, "slow"),
                                                       (("s32", "h32", "h32_generic"), "bf16", True, "fast"),
                                                       (("wp64", "wp64_grouped", "wp64_forced"), "f32", True, "fast"),
                                                       (("wp64", "wp64_grouped"), "bf16", False, "slow")])
def test_finalize_forms_give_identical_bits_at_a_late_step(routes, weights, slab, hyper):
    """Hidden 32: step_finalize_s32, step_finalize_h32 and step_finalize; hidden 64: step_finalize_ws with one thread per quad and
    grouped - the same adamw_elem on the same inputs must give the same bits of p, m and v.  Nine objects, step 5000, non-default
    hyper-parameters (from zero moments at step 1 most of a wrong form would not show)."""
    n = 9
    if "wp64" in routes:
        assert _one_thread_per_quad("wp64", n) and not _one_thread_per_quad("wp64_grouped", n)
    outs = [_one_update(r, n, weights, slab, 4242, hyper, 4999) for r in routes]
    for r, o in zip(routes[1:], outs[1:]):
        for key, a, b in zip("pmv", outs[0], o):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{key}: {routes[0]} and {r} differ"


SPECIAL_G = np.array([0.0, 1e-40, -1e-40, 1e-30, -1e-30, 1e20, -1e20], np.float32)


@pytest.mark.parametrize("route", list(ROUTES))
def test_special_gradient_values(route):
    """Gradients 0, +-1e-40 (subnormal), +-1e-30 (g g underflows), +-1e20 (g g overflows: v = inf, denom = inf, the update is 0 and
    p' = p decay, as in torch), each against zero and non-zero (m, v).  Float64 is the wrong model here: the comparison is the
    float32 op-by-op evaluation - the same finiteness class per element, finite values within the rounding bound plus FLT_MIN (a
    flush of subnormals is tolerated, nothing else).  Then one NaN and one inf in the real part of the gradient slab: exactly those
    elements of p, m, v become non-finite; their quad neighbours and every other object stay within the bound."""
    n = 3
    fx = _Fixture(route, n, "f32", False, "default", 999, seed=77)
    P, hp = fx.P, fx.hp
    rng = np.random.default_rng(78)
    p0, _, m0, v0 = ar.make_inputs(rng, (n, P))
    idx = np.arange(n * P).reshape(n, P)
    g = SPECIAL_G[idx % 7]
    zero = (idx // 7) % 2 == 0                       # every gradient value meets zero and non-zero moments
    m0[zero], v0[zero] = 0.0, 0.0
    sub = ((idx // 14) % 3 == 1) & ~zero             # ... and moments in the subnormal range
    m0[sub], v0[sub] = np.float32(3e-41), np.float32(2e-42)
    fx.set_params(p0)
    fx.set_moments(m0, v0)
    fx.apply(g)
    p1, (m1, v1) = fx.params(), fx.moments()
    fx.assert_untouched()
    ep, em, ev = _f32_emulation(p0, g, m0, v0, 1000, hp)
    _, _, _, tol_p, tol_m, tol_v = ar.adamw_f64(p0, g, m0, v0, 1000, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
    big = np.abs(g) == np.float32(1e20)
    assert np.isinf(ev[big]).all() and np.isfinite(ep).all() and np.array_equal(ep[big], (p0 * ar.adamw_constants(1000, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])["decay"])[big])
    for key, got, emu, tol in (("m", m1[:, :P], em, tol_m), ("v", v1[:, :P], ev, tol_v), ("p", p1, ep, tol_p)):
        fin = np.isfinite(emu)
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(emu)), f"{route}: finiteness of {key}"
        assert np.array_equal(got[~fin], emu[~fin]), f"{route}: {key} where it is infinite"
        _assert_within(got, emu.astype(np.float64), tol + ar.FLT_MIN, f"{route}: {key}", P, mask=fin)

    # one NaN and one inf among the real gradients: in the middle of a quad of object 0, in the last (partly padded) quad of object 2
    p0 = fx.params()
    m0, v0 = (a[:, :P] for a in fx.moments())
    m0, v0 = np.where(np.isfinite(m0), m0, 1.0).astype(np.float32), np.where(np.isfinite(v0), v0, 1.0).astype(np.float32)
    fx.set_moments(m0, v0)
    g = ar.make_gradients(rng, (n, P))
    at_nan, at_inf = (0, 4 * (P // 8) + 1), (2, P - 1)
    g[at_nan], g[at_inf] = np.nan, np.inf
    fx.apply(g)
    p1, (m1, v1) = fx.params(), fx.moments()
    fx.assert_untouched()
    hit = np.zeros((n, P), bool)
    hit[at_nan] = hit[at_inf] = True
    rp, rm, rv, tol_p, tol_m, tol_v = ar.adamw_f64(p0, np.where(hit, 0.0, g), m0, v0, 1001, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
    for key, got, ref, tol in (("m", m1[:, :P], rm, tol_m), ("v", v1[:, :P], rv, tol_v), ("p", p1, rp, tol_p)):
        assert np.array_equal(~np.isfinite(got), hit), f"{route}: non-finite {key} at {np.argwhere(~np.isfinite(got) != hit)[:4].tolist()}"
        _assert_within(got, ref, tol, f"{route}: {key} next to a non-finite gradient", P, mask=~hit)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("weights", ["f32", "bf16"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_image_rewritten_by_adamw_apply_equals_a_fresh_pack(route, weights):
    """prepare_frame -> adamw_apply (late step, non-zero moments) -> fwd_bwd(prepared_step=0) reads the image the finalize just
    rewrote element by element; a fresh operator given the updated parameters packs it anew.  Loss, renders and all gradients bit for
    bit: an element written to the wrong image position, or rounded differently (bf16), would show in either."""
    H = ROUTES[route][0]
    if H == 32:
        c = cases.build_case("tiny")
        n, params, batch = c["n"], (c["fc"], c["B"], c["scale"]), c["batch"]
    else:
        n, params, batch = 3, synth.make_params(3, H, seed=700 + H), synth.make_batch(3, R, S, seed=701 + H)
    fx = _Fixture(route, n, weights, False, "default", 999, params=params, batch=batch)
    rng = np.random.default_rng(702 + H)
    P = fx.P
    # moments with |m| <~ sqrt(v): every parameter moves by a few lr at most and the field stays a field
    s = 10.0 ** rng.uniform(-6.0, 0.0, (n, P))
    g = (rng.normal(0, 1, (n, P)) * s).astype(np.float32)
    fx.set_moments((rng.normal(0, 1, (n, P)) * s).astype(np.float32), (((np.abs(rng.normal(0, 1, (n, P))) + 0.5) * s) ** 2).astype(np.float32))
    before = fx.params()
    fx.apply(g)
    assert not np.array_equal(before, fx.params())

    def run(op, **kw):
        gfc = [torch.full_like(t, float("nan")) for t in fx.fc]
        gB = torch.full_like(fx.B, float("nan"))
        res = op.fwd_bwd(fx.fc, fx.B, fx.sc, *fx.args(), grads_fc=gfc, grad_B=gB, render=True, **kw)
        torch.cuda.synchronize()
        return [res.loss, res.render_depth, res.render_color, res.opacity, res.var] + gfc + [gB]

    kept = run(fx.op, prepared_step=0)
    fresh = run(make_op(n, R, S, H, device=DEV, max_steps=1, weights=weights, tuning=ROUTES[route][1]))
    assert bool(torch.isfinite(kept[0]).all())
    names = ["loss", "render_depth", "render_color", "opacity", "var"] + [f"g_fc{t}" for t in range(14)] + ["g_B"]
    for name, a, b in zip(names, kept, fresh):
        assert bool(torch.isfinite(a).all()), name
        assert _bits_equal(a, b), f"{route} {weights}: {name} differs between the rewritten and the freshly packed image"


@pytest.mark.parametrize("name,tuning", [("tiny", None), ("tiny", {"kernel": _lib.KERNEL_H32_F32}), ("h64", None)])
def test_device_step_table_at_and_past_its_last_entry(name, tuning):
    """The device-side table of the two step-dependent constants is indexed with min(count + i, len - 1).  With betas (0.5, 0.9) it
    saturates after some 160 entries: a state three steps short of its end runs two calls of three steps - across the last entry and
    on beyond it - against a state without the table (the host forms the constants of every step): losses, parameters and moments
    bit for bit, and the device count equals the host count."""
    c = cases.build_case(name)
    n, H = c["n"], c["H"]
    rng = np.random.default_rng(900)
    P = layout.param_count(H)
    s = 10.0 ** rng.uniform(-6.0, 0.0, (n, P))
    m0 = (rng.normal(0, 1, (n, P)) * s).astype(np.float32)
    v0 = (((np.abs(rng.normal(0, 1, (n, P))) + 0.5) * s) ** 2).astype(np.float32)
    hyper = dict(lr=1e-3, betas=(0.5, 0.9), eps=1e-8, weight_decay=0.013)
    probe = step.FusedAdamWState(1, H, DEV, **hyper)
    probe.enable_device_steps()
    length = int(probe.bias_table.shape[0])          # the real length, whatever it is
    assert 100 < length < 400, length
    outs = []
    for device_steps in (True, False):
        fc = [torch.from_numpy(a).to(DEV) for a in c["fc"]]
        B, sc = torch.from_numpy(c["B"]).to(DEV), torch.from_numpy(c["scale"]).to(DEV)
        b = {k: torch.from_numpy(v).to(DEV) for k, v in c["batch"].items()}
        frame = {k: torch.cat([v.roll(i, dims=1) for i in range(3)], dim=1).contiguous() for k, v in b.items()}
        args = (frame["pcs"], frame["z"], frame["gt_depth"], frame["gt_rgb"], frame["sem"], frame["depth_mask"])
        op = make_op(n, c["R"], c["S"], H, device=DEV, max_steps=3, tuning=tuning)
        st = step.FusedAdamWState(n, H, DEV, **hyper)
        st.exp_avg[:, :P].copy_(torch.from_numpy(m0).to(DEV))
        st.exp_avg_sq[:, :P].copy_(torch.from_numpy(v0).to(DEV))
        st.step = length - 3
        if device_steps:
            st.enable_device_steps()
            assert int(st.bias_table.shape[0]) == length and int(st.step_counter.sum()) == length - 3
        losses = [op.train_steps(fc, B, sc, *args, opt=st, n_steps=3).loss.clone() for _ in range(2)]
        torch.cuda.synchronize()
        assert st.step == length + 3
        if device_steps:
            assert int(st.step_counter.sum()) == st.step
        outs.append((torch.cat(losses), [t.clone() for t in fc + [B]], st.exp_avg.clone(), st.exp_avg_sq.clone()))
    (la, pa, ma, va), (lb, pb, mb, vb) = outs
    assert bool(torch.isfinite(la).all())
    assert _bits_equal(la, lb)
    for x, y in zip(pa, pb):
        assert _bits_equal(x, y)
    assert _bits_equal(ma, mb) and _bits_equal(va, vb)
