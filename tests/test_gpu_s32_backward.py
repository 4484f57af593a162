"""GPU tier: the backward of step_main_s32 transposes its weight-gradient operands on two alternating result tiles, ties the mask / split
chunks of mid1 / mid2 and the d(projection) products where the source forms them, and (one pass per workgroup) writes the bias sums, the
head gradients and the B_layer.weight sums into their cleared cells without reading them; the measurement build keeps the former backward -
the former source in a template instantiation of its own - behind tuning.ws_flags bit 6.  Every value is computed by the same operations
on the same operands in the same order, so loss, flags, renders, var and all 15 gradients of the PRODUCT must be the same BYTES as the
former backward's: on the shapes of test_gpu_s32_front.py (one ray, a partial last tile, a nearly empty second ray group, an exactly full
group, many objects, the longest ray of the 16-lane compositing, bf16 weights, the six-product backward), on the smallest shape the
planner gives the multi-pass form (which keeps the read-modify-writes), and on the fixtures with exactly zero gradients.

The zero-cell writes store 0.0f + x where the former backward adds x to a cleared cell: the case to guard is a sum that is exactly zero
(a negative zero must come out as +0.0f both ways).  On the CPU oracle none of the drop_* / saturated / exact_hit fixtures gives an
all-zero mid1 or mid2 bias gradient, not for a workgroup and not for an object (the opacity term reaches both layers through the alpha
head whatever the masks drop); drop_colour and exact_hit give exactly zero colour-head gradients (out_color weight and bias, color_linear)
for every object, so the head cells written the same way are all zero there, and the test checks that they are."""
import numpy as np
import pytest
import torch

import cases
from conftest import AB_LIBRARY, GRAD_KEYS, RENDER_KEYS
from test_gpu_parity import DEV, _run
from vmap_amd import _lib, step, synth

pytestmark = pytest.mark.gpu

FORMER = {"ws_flags": 64}
# (n, R, S, weights, tuning)
SHAPES = [(1, 1, 10, "f32", {}), (2, 5, 10, "f32", {}), (3, 13, 10, "f32", {}), (2, 12, 10, "f32", {}), (40, 24, 10, "f32", {}),
          (2, 3, 16, "f32", {}), (2, 12, 10, "bf16", {}), (2, 12, 10, "f32", {"kernel": _lib.KERNEL_S32_BWD6})]


def _tobytes(a):
    return np.ascontiguousarray(a).tobytes()


def _same_bytes(c, weights="f32", tuning=None):
    tuning = dict(tuning or {})
    n, R, S = c["n"], c["R"], c["S"]
    new = _run(c, op=step.VmapStep(n, R, S, 32, device=DEV, weights=weights, tuning=tuning or None))
    old = _run(c, op=step.VmapStep(n, R, S, 32, device=DEV, weights=weights, tuning={**tuning, **FORMER}, library=AB_LIBRARY))
    assert np.isfinite(new["g_B"]).all() and np.abs(new["g_B"]).max() > 0
    assert np.float32(new["loss"]).tobytes() == np.float32(old["loss"]).tobytes()
    assert _tobytes(new["flags"]) == _tobytes(old["flags"])
    for k in RENDER_KEYS + ["var"] + GRAD_KEYS:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and _tobytes(new[k]) == _tobytes(old[k]), k
    return new


def _synth_case(n, R, S):
    fc, B, sc = synth.make_params(n, 32, scale=2.0, seed=700 + R)
    return dict(n=n, R=R, S=S, H=32, fc=fc, B=B, scale=sc, batch=synth.make_batch(n, R, S, seed=800 + R + S))


@pytest.mark.parametrize("n,R,S,weights,tuning", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_product_gives_the_bytes_of_the_former_backward(n, R, S, weights, tuning):
    _same_bytes(_synth_case(n, R, S), weights, tuning)


def _smallest_multipass_shape(S=10):
    """the fewest points (n * R) at which the planner gives step_main_s32 more rounds than workgroups per object"""
    best = None
    for n in range(1, 260):
        for R in range(1, 64):
            if best is not None and n * R >= best[0] * best[1]:
                break
            p = _lib.describe_plan(n, R, S, 32)
            if p["kernel"] == "step_main_s32" and not p["single_round"] and p["rounds_per_object"] > p["workgroups_per_object"]:
                best = (n, R)
                break
    assert best is not None
    return best


def test_multipass_form_gives_the_bytes_of_the_former_backward():
    n, R = _smallest_multipass_shape()
    p = _lib.describe_plan(n, R, 10, 32)
    print("smallest multi-pass shape:", (n, R, 10), p)
    assert p["rounds_per_object"] > p["workgroups_per_object"] and not p["single_round"]
    _same_bytes(_synth_case(n, R, 10))


@pytest.mark.parametrize("name", ["drop_colour", "exact_hit", "drop_opacity", "drop_depth", "saturated"])
def test_fixtures_with_zero_sums_give_the_bytes_of_the_former_backward(name):
    c = cases.build_case(name)
    new = _same_bytes(c)
    if name in ("drop_colour", "exact_hit"):       # color_linear and out_color: exactly zero, and +0.0f, in every cell
        for k in ("g_fc10", "g_fc11", "g_fc12", "g_fc13"):
            assert _tobytes(new[k]) == bytes(new[k].nbytes), k


def test_three_training_steps_leave_the_same_parameters():
    n, R, S, steps = 2, 12, 10, 3
    fc0, B0, sc = synth.make_params(n, 32, scale=2.0, seed=712)
    frame = synth.make_batch(n, R * steps, S, seed=812)
    fr = tuple(torch.from_numpy(frame[k]).to(DEV) for k in ("pcs", "z", "gt_depth", "gt_rgb", "sem", "depth_mask"))
    outs = []
    for extra, lib in ((None, None), (FORMER, AB_LIBRARY)):
        fc = [torch.from_numpy(a.copy()).to(DEV) for a in fc0]
        B, tsc = torch.from_numpy(B0.copy()).to(DEV), torch.from_numpy(sc).to(DEV)
        op = step.VmapStep(n, R, S, 32, device=DEV, max_steps=steps, tuning=extra, **({"library": lib} if lib else {}))
        res = op.train_steps(fc, B, tsc, *fr, opt=step.FusedAdamWState(n, 32, DEV, lr=1e-3, weight_decay=0.013), n_steps=steps, ray_step=R)
        torch.cuda.synchronize()
        outs.append([res.loss.cpu().numpy()[:steps]] + [t.cpu().numpy() for t in fc] + [B.cpu().numpy()])
    assert len(outs[0]) == 16                              # the losses + the 15 parameter tensors
    assert not np.array_equal(outs[0][1], fc0[0])          # the steps did move the parameters
    for a, b in zip(*outs):
        assert _tobytes(a) == _tobytes(b)


def test_former_backward_ships_in_the_measurement_build_only():
    with pytest.raises(_lib.VmapStepError, match="measurement build only"):
        step.VmapStep(2, 12, 10, 32, device=DEV, tuning=FORMER)
