"""CPU tier: the float64 AdamW reference of tests/adamw_ref.py and its rounding bounds, checked against the float32 op-by-op
evaluation of the same update (oracle.vmap_oracle.adamw_update) - the bounds must hold for a CORRECT float32 implementation with
room to spare, and must not hold for the two classic wrong ones.  Keeps the bounds honest if someone later widens them."""
import numpy as np
import pytest

import adamw_ref as ar
from oracle import vmap_oracle as vo

STEPS = (1, 2, 3, 10, 100, 1000, 20001, 100000)
N = 200_000


def _f32_emulation(p, g, m, v, step, hp, **kw):
    # the hyper-parameters as the C ABI carries them (float32, widened): the emulation then forms the same seven constants
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in (hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"]))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        return vo.adamw_update(p, g, m, v, step, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, dtype=np.float32, **kw)


@pytest.mark.parametrize("hyper", list(ar.HYPER))
def test_float32_emulation_stays_inside_the_rounding_bounds(hyper):
    hp = ar.HYPER[hyper]
    rng = np.random.default_rng(20 + list(ar.HYPER).index(hyper))
    p, g, m, v = ar.make_inputs(rng, (N,))
    assert (g == 0).mean() > 0.03 and ((m == 0) & (v == 0)).mean() > 0.03          # the exact zeros are there
    top = np.zeros(3)
    for step in STEPS:
        pe, me, ve = _f32_emulation(p, g, m, v, step, hp)
        p1, m1, v1, tol_p, tol_m, tol_v = ar.adamw_f64(p, g, m, v, step, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
        assert np.isfinite(p1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
        use = [ar.worst(me, m1, tol_m)[0], ar.worst(ve, v1, tol_v)[0], ar.worst(pe, p1, tol_p)[0]]
        top = np.maximum(top, use)
        assert max(use) < 1.0, (hyper, step, use)
    print(f"{hyper}: float32 emulation uses at most {top[0]:.2f} / {top[1]:.2f} / {top[2]:.2f} of tol_m / tol_v / tol_p")
    # a correct implementation has room, so a bound that is met is not met by luck
    assert top.max() < 0.8


def test_constants_are_formed_in_double_and_rounded_once():
    c = ar.adamw_constants(1000, **{k if k != "weight_decay" else "wd": x for k, x in ar.HYPER["default"].items()})
    lr, b1, b2 = float(np.float32(1e-3)), float(np.float32(0.9)), float(np.float32(0.999))
    assert c["decay"] == np.float32(1.0 - lr * float(np.float32(0.013)))
    assert c["one_minus_beta1"] == np.float32(1.0 - b1) and c["one_minus_beta1"] != np.float32(1.0 - 0.9)      # beta1 travels as float32
    assert c["beta2"] == np.float32(0.999) and c["one_minus_beta2"] == np.float32(1.0 - b2)
    assert c["step_size"] == np.float32(lr / (1.0 - b1 ** 1000)) and c["bias_corr2_sqrt"] == np.float32(np.sqrt(1.0 - b2 ** 1000))
    # step 1 from zero moments: the update is lr * g / (|g| + eps) whatever the betas are - the blind spot of a zero-state test
    g = np.array([0.5, -2.0, 1e-3], np.float32)
    z = np.zeros(3, np.float32)
    for hp in ar.HYPER.values():
        p1, m1, v1, *_ = ar.adamw_f64(z, g, z, z, 1, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
        lr32, eps32 = float(np.float32(hp["lr"])), float(np.float32(hp["eps"]))
        assert np.allclose(p1, -lr32 * g / (np.abs(g) + eps32), rtol=1e-6, atol=0)


def _wrong_eps_inside_root(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, dtype):
    p, g, m, v = (a.astype(dtype) for a in (p, g, m, v))
    p = p * dtype(1.0 - lr * weight_decay)
    m = m + (g - m) * dtype(1.0 - beta1)
    v = v * dtype(beta2) + g * g * dtype(1.0 - beta2)
    denom = np.sqrt(v + dtype(eps)) / dtype(np.sqrt(1.0 - beta2 ** step))
    return (p - dtype(lr / (1.0 - beta1 ** step)) * (m / denom)).astype(dtype), m, v


@pytest.mark.parametrize("hyper", list(ar.HYPER))
def test_bounds_reject_the_classic_wrong_updates(hyper):
    """eps under the root, beta2 swapped with 1 - beta2, a bias correction of the step before: each leaves most elements of the
    input family outside the bound (a max-norm or quantile check of |dp| <= steps * lr would pass all three)."""
    hp = ar.HYPER[hyper]
    rng = np.random.default_rng(77)
    p, g, m, v = ar.make_inputs(rng, (20_000,))
    step = 1000
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in (hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"]))
    p1, m1, v1, tol_p, tol_m, tol_v = ar.adamw_f64(p, g, m, v, step, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
    with np.errstate(all="ignore"):
        pw, _, _ = _wrong_eps_inside_root(p, g, m, v, step, lr, b1, b2, eps, wd, np.float32)
        assert (ar.bound_use(pw, p1, tol_p) > 1.0).mean() > 0.1
        _, _, vw = vo.adamw_update(p, g, m, v, step, lr=lr, beta1=b1, beta2=1.0 - b2, eps=eps, weight_decay=wd, dtype=np.float32)
        assert (ar.bound_use(vw, v1, tol_v) > 1.0).mean() > 0.5
        pw, _, _ = vo.adamw_update(p, g, m, v, step - 1, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, dtype=np.float32)
        if hyper != "fast":          # beta2 = 0.9: 0.9^1000 is gone, both steps have the same corrections
            assert (ar.bound_use(pw, p1, tol_p) > 1.0).mean() > 0.1
