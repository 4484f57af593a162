"""CPU tier, siblings of the three zero-state AdamW tests of tests/test_kernel_sim.py: the optimiser arithmetic of every finalize
form at a LATE step from NON-ZERO moments, on the CPU executor.

From zero moments at step 1 the update is lr * g / (|g| + eps) whatever beta1, beta2 and the two bias corrections are, and every
moment read returns the same zero whatever its address: those tests cannot see the decay of either moment, the corrections or the
moment read path.  Here the kernels' own source runs the step, the finalize sums its gradients, and p, m, v are held element by
element to the float64 update on those gradients within the rounding bounds of tests/adamw_ref.py.  The executor's harness hands
vl::adamw_consts lr 1e-3, weight decay 0.013, eps 1e-8 as float32 and the betas as the double literals 0.9 / 0.999
(tests/sim/sim_abi.cpp) - the reference forms its constants from exactly those (``betas_as_float32=False``); on the device, where the
betas cross the ABI as float32, tests/test_gpu_adamw.py does the same with three hyper-parameter sets."""
import numpy as np
import pytest

import adamw_ref as ar
import cases
import simlib

STEP = 1000


def _flat_params(fc, B):
    n = B.shape[0]
    return np.concatenate([np.asarray(a, np.float32).reshape(n, -1) for a in fc] + [np.asarray(B, np.float32).reshape(n, -1)], axis=1)


def _late_adam_state(flat, seed):
    """Parameters + seeded non-zero moments over eight decades (a few exact zeros among them), the padding columns of the moment
    slabs filled with a pattern no update produces, the step count of a run long under way."""
    n, P = flat.shape
    PP = (P + 63) // 64 * 64
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-7.0, 1.0, (n, P))
    m = np.empty((n, PP), np.float32)
    v = np.empty((n, PP), np.float32)
    m[:, :P] = rng.normal(0.0, 1.0, (n, P)) * scale
    v[:, :P] = (rng.normal(0.0, 1.0, (n, P)) * scale * 10.0 ** rng.uniform(-1.0, 1.0, (n, P))) ** 2
    z = rng.random((n, P)) < 0.02
    m[:, :P][z] = 0.0
    v[:, :P][z] = 0.0
    m[:, P:] = -7.25 - np.arange(PP - P, dtype=np.float32)[None, :] - 100.0 * np.arange(n, dtype=np.float32)[:, None]
    v[:, P:] = 3.5 + np.arange(PP - P, dtype=np.float32)[None, :] + 100.0 * np.arange(n, dtype=np.float32)[:, None]
    assert not np.isnan(m).any() and not np.isnan(v).any()
    return dict(p=flat.copy(), m=m, v=v, step=STEP)


def _run_and_check(what, *sim_args, seed, flat, **kw):
    """One simulated step with the fused update from a late state; every element of p, m, v within its rounding bound of the float64
    update on the gradients the finalize summed, the moment padding bit-unchanged.  -> the state after the step"""
    state = _late_adam_state(flat, seed)
    before = {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in state.items()}
    s = simlib.sim_step(*sim_args, adam=state, **kw)
    gflat = s["grads_flat"]
    n, P = flat.shape
    assert np.isfinite(gflat).all() and np.any(gflat != 0)
    hp = ar.HYPER["default"]
    p1, m1, v1, tol_p, tol_m, tol_v = ar.adamw_f64(before["p"], gflat[:, :P], before["m"][:, :P], before["v"][:, :P], STEP, hp["lr"],
                                                   hp["betas"], hp["eps"], hp["weight_decay"], betas_as_float32=False)
    for key, got, ref, tol in (("m", state["m"][:, :P], m1, tol_m), ("v", state["v"][:, :P], v1, tol_v), ("p", state["p"], p1, tol_p)):
        use, i = ar.worst(got, ref, tol)
        assert use <= 1.0, f"{what}: {key}[{i // P}, {i % P}] is {use:.3g} of its rounding bound from the float64 update"
    for key in ("m", "v"):
        assert np.array_equal(state[key][:, P:].view(np.uint32), before[key][:, P:].view(np.uint32)), f"{what}: padding of {key} written"
    return state


@pytest.mark.parametrize("name,kw", [("tiny", {}), ("tiny", dict(split=True)), ("ragged", dict(split=True, NW=2, G=5)), ("h64", {}),
                                     ("bg_h128_s14", dict(wide=4, NW=5, finalize_form=0)), ("bg_h128_s14", dict(wide=4, NW=5, finalize_form=1)),
                                     ("h64", dict(wide=4, NW=2, finalize_form=0)), ("h64", dict(wide=4, NW=2, finalize_form=1))])
def test_sim_fused_adamw_late_step_matches_float64_update(name, kw):
    """adamw_elem as every finalize form inlines it - step_finalize_h32 (tiny), step_finalize_s32 (split), step_finalize (h64 on the
    general kernel), step_finalize_ws grouped and with one thread per quad (hidden 128 / 64) - at step 1000 from non-zero moments."""
    c = cases.build_case(name)
    _run_and_check(f"{name} {kw}", c, seed=31, flat=_flat_params(c["fc"], c["B"]), **kw)


def test_sim_ws_fused_adamw_late_step_with_nine_objects_on_the_xcd_affine_map():
    """Nine objects: step_finalize_ws deals its blocks to the objects in groups of eight and seven blocks of the second group exit
    early - every object's moments must still be read at ITS offset (from zero moments a wrong offset reads the same zeros).  Both
    thread forms: the float64 update within the bounds, and the same bits from either."""
    from vmap_amd import synth
    n, R, S, H = 9, 6, 10, 64
    fc, B, sc = synth.make_params(n, H, seed=91)
    batch = synth.make_batch(n, R, S, seed=92)
    outs = [_run_and_check(f"nine objects, form {form}", fc, B, sc, batch, seed=33, flat=_flat_params(fc, B), wide=4, NW=1, finalize_form=form)
            for form in (0, 1)]
    for k in ("p", "m", "v"):
        assert np.array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32)), k
