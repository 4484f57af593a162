"""TEST INFRASTRUCTURE: torch.optim.AdamW's single-tensor update in float64 on float32 inputs, the rounding bounds a float32
evaluation of it must meet, and the seeded inputs the optimiser tests share.  Plain numpy; nothing of ``vmap_amd`` is imported.

The kernels restate ``_single_tensor_adamw`` (torch/optim/adamw.py) element by element (``adamw_elem``, csrc/step_kernels.h) with
seven constants the host forms in double and rounds ONCE to float32 (``vl::adamw_consts``, csrc/step_plan.h).  The reference takes
exactly those seven float32 constants - they are inputs of the operation, not part of its error - and evaluates the update in
float64.  The bounds count the float32 roundings of ``adamw_elem`` (u = 2^-24 per operation):

  m' = m + (g - m) c1             three roundings of magnitudes <= |m| + |g|                  tol_m = 3u (|m| + |g|)
  v' = v b2 + (g g) c2            four roundings of non-negative terms, each <= v'            tol_v = 4u v'
  p' = p decay - ss (m' / denom)  p decay and the final difference: 2 roundings of ~|p| (+ the update's share, 4u |p| in all);
                                  sqrt, /bc2, +eps, m'/denom, ss*: 5 roundings + the errors of m' (3u) and of v' under the root
                                  (2u), relative to ss (|m| + |g|) / denom                   tol_p = 4u |p| + 8u ss (|m| + |g|) / denom

each plus one float32 subnormal (2^-149) for results that round in the subnormal range.  They are conditions derived from the
operation count, not measurements; tests/test_adamw_ref.py checks that a float32 op-by-op evaluation stays inside them.
"""
import math

import numpy as np

U = 2.0 ** -24                 # unit roundoff of float32
SUBNORMAL = 2.0 ** -149        # the smallest float32 subnormal
FLT_MIN = 2.0 ** -126          # the smallest normal float32

# the hyper-parameter sets of the optimiser tests: the defaults of FusedAdamWState and two sets that move every constant
HYPER = {
    "default": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.013),
    "fast": dict(lr=3e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.0),
    "slow": dict(lr=1e-4, betas=(0.95, 0.9999), eps=1e-10, weight_decay=0.5),
}


def adamw_constants(step_after, lr, betas, eps, wd, betas_as_float32=True):
    """The seven float32 constants of one update as vl::adamw_consts forms them: the hyper-parameters travel as float32
    (vmapstep_adamw), are widened to double, combined in double and rounded once.  -> dict of np.float32
    ``betas_as_float32=False``: the betas reach vl::adamw_consts as the doubles they are - what the CPU executor's harness does
    (tests/sim/sim_abi.cpp hands it the literals 0.9 and 0.999; lr, eps and the weight decay are float32 there too)."""
    lr, wd = float(np.float32(lr)), float(np.float32(wd))
    b1, b2 = (float(np.float32(b)) if betas_as_float32 else float(b) for b in betas)
    t = float(int(step_after))
    return dict(decay=np.float32(1.0 - lr * wd), one_minus_beta1=np.float32(1.0 - b1), beta2=np.float32(b2),
                one_minus_beta2=np.float32(1.0 - b2), eps=np.float32(eps),
                step_size=np.float32(lr / (1.0 - math.pow(b1, t))), bias_corr2_sqrt=np.float32(math.sqrt(1.0 - math.pow(b2, t))))


def adamw_f64(p, g, m, v, step_after, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.013, betas_as_float32=True):
    """One AdamW update in float64 on float32 inputs.  ``step_after``: the 1-based step count after the increment.
    -> (p', m', v', tol_p, tol_m, tol_v), all float64, the tolerances per element."""
    c = {k: float(x) for k, x in adamw_constants(step_after, lr, betas, eps, wd, betas_as_float32).items()}
    p, g, m, v = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, g, m, v))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        p1 = p * c["decay"]                                                   # param.mul_(1 - lr * wd)
        m1 = m + (g - m) * c["one_minus_beta1"]                               # exp_avg.lerp_(grad, 1 - beta1)
        v1 = v * c["beta2"] + (g * g) * c["one_minus_beta2"]                  # exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
        denom = np.sqrt(v1) / c["bias_corr2_sqrt"] + c["eps"]
        p1 = p1 - c["step_size"] * (m1 / denom)                               # param.addcdiv_(exp_avg, denom, -lr / bc1)
        mag = np.abs(m) + np.abs(g)
        tol_m = 3.0 * U * mag + SUBNORMAL
        tol_v = 4.0 * U * v1 + SUBNORMAL
        tol_p = 4.0 * U * np.abs(p) + 8.0 * U * c["step_size"] * mag / denom + SUBNORMAL
    return p1, m1, v1, tol_p, tol_m, tol_v


def make_inputs(rng, shape):
    """The seeded input family of the optimiser tests: parameters N(0, 0.3); gradients and moments over fifteen decades (a
    per-element scale 10^U(-12, 3)), moments up to a hundred times below and ten times above the gradient's scale; 5 % of the
    gradients and 5 % of the (m, v) pairs exactly zero.  -> float32 (p, g, m, v)"""
    p = rng.normal(0.0, 0.3, shape)
    scale = 10.0 ** rng.uniform(-12.0, 3.0, shape)
    g = rng.normal(0.0, 1.0, shape) * scale
    m = rng.normal(0.0, 1.0, shape) * scale * 10.0 ** rng.uniform(-2.0, 1.0, shape)
    v = (rng.normal(0.0, 1.0, shape) * scale * 10.0 ** rng.uniform(-2.0, 1.0, shape)) ** 2
    g[rng.random(shape) < 0.05] = 0.0
    z = rng.random(shape) < 0.05
    m[z] = 0.0
    v[z] = 0.0
    return tuple(a.astype(np.float32) for a in (p, g, m, v))


def make_gradients(rng, shape):
    """fresh gradients of the same family (for the second and third call of a case)"""
    g = rng.normal(0.0, 1.0, shape) * 10.0 ** rng.uniform(-12.0, 3.0, shape)
    g[rng.random(shape) < 0.05] = 0.0
    return g.astype(np.float32)


def bound_use(got, ref, tol):
    """per element |got - ref| / tol (float64)"""
    with np.errstate(invalid="ignore"):            # inf - inf where both are infinite: NaN, which no caller counts as inside
        return np.abs(np.asarray(got, dtype=np.float64) - ref) / tol


def worst(got, ref, tol):
    """(largest share of the bound any element uses, its flat index) - for assertion messages; a NaN counts as infinitely far"""
    r = bound_use(got, ref, tol).ravel()
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r)) if r.size else 0
    return (float(r[i]) if r.size else 0.0), i
