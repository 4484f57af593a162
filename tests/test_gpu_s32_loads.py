"""GPU tier: step_main_s32 requests B_layer.weight in front of the image copy, the per-object switches / normalisers as two 16-byte
loads and the sample's z with the per-ray loads, all in front of the MLP forward; the measurement build keeps the former load order
- the former source in a template instantiation of its own - behind tuning.ws_flags bit 4.  No arithmetic moved, so loss, flags,
renders, var and all 15 gradients must be the same BITS in both forms of the measurement build, on shapes with padding lanes (the
guarded z), partly filled ray groups, several passes per workgroup, bf16 weights and set empty-mask switches."""
import numpy as np
import pytest
import torch

import cases
from conftest import AB_LIBRARY, GRAD_KEYS, RENDER_KEYS
from test_gpu_parity import DEV, _run
from vmap_amd import _lib, step, synth

pytestmark = pytest.mark.gpu

OLD_ORDER = {"ws_flags": 16}
# (n, R, S, weights, tuning): one ray and 118 padding lanes; a second ray group holding one ray; a full group; other sample counts;
# workgroups_per_object = 1 -> the MULTI instantiation, three passes, the last with one ray; bf16 weights
SHAPES = [(1, 1, 10, "f32", {}), (2, 5, 10, "f32", {}), (3, 13, 10, "f32", {}), (2, 12, 10, "f32", {}), (2, 12, 16, "f32", {}),
          (2, 12, 7, "f32", {}), (2, 25, 10, "f32", {"workgroups_per_object": 1}), (2, 12, 10, "bf16", {})]


def _both(c, weights="f32", tuning=None):
    ops = [step.VmapStep(c["n"], c["R"], c["S"], 32, device=DEV, weights=weights, tuning={**(tuning or {}), **extra} or None, library=AB_LIBRARY)
           for extra in ({}, OLD_ORDER)]
    return [_run(c, op=op) for op in ops]


def _same_bits(new, old):
    assert np.isfinite(new["g_B"]).all() and np.abs(new["g_B"]).max() > 0
    assert new["loss"] == old["loss"] and np.array_equal(new["flags"], old["flags"])
    for k in RENDER_KEYS + ["var"] + GRAD_KEYS:
        assert np.array_equal(new[k], old[k]), k


@pytest.mark.parametrize("n,R,S,weights,tuning", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_new_load_order_gives_the_bits_of_the_old_one(n, R, S, weights, tuning):
    fc, B, sc = synth.make_params(n, 32, scale=2.0, seed=500 + R)
    batch = synth.make_batch(n, R, S, seed=600 + R + S)
    new, old = _both(dict(n=n, R=R, S=S, H=32, fc=fc, B=B, scale=sc, batch=batch), weights, tuning)
    _same_bits(new, old)


@pytest.mark.parametrize("name,flag", [("drop_depth", 0), ("drop_colour", 1), ("drop_opacity", 2)])
def test_a_set_switch_still_zeroes_its_normaliser(name, flag):
    c = cases.build_case(name)
    new, old = _both(c)
    assert new["flags"][flag] != 0          # the fixture's masks do set the switch
    _same_bits(new, old)
    prod = _run(c, op=step.VmapStep(c["n"], c["R"], c["S"], 32, device=DEV))          # the product library: the same bits again
    _same_bits(prod, old)


def test_three_training_steps_leave_the_same_parameters():
    n, R, S, steps = 2, 12, 10, 3
    fc0, B0, sc = synth.make_params(n, 32, scale=2.0, seed=512)
    frame = synth.make_batch(n, R * steps, S, seed=612)
    fr = tuple(torch.from_numpy(frame[k]).to(DEV) for k in ("pcs", "z", "gt_depth", "gt_rgb", "sem", "depth_mask"))
    outs = []
    for extra in (None, OLD_ORDER):
        fc = [torch.from_numpy(a.copy()).to(DEV) for a in fc0]
        B, tsc = torch.from_numpy(B0.copy()).to(DEV), torch.from_numpy(sc).to(DEV)
        op = step.VmapStep(n, R, S, 32, device=DEV, max_steps=steps, tuning=extra, library=AB_LIBRARY)
        res = op.train_steps(fc, B, tsc, *fr, opt=step.FusedAdamWState(n, 32, DEV, lr=1e-3, weight_decay=0.013), n_steps=steps, ray_step=R)
        torch.cuda.synchronize()
        outs.append([res.loss.cpu().numpy()[:steps]] + [t.cpu().numpy() for t in fc] + [B.cpu().numpy()])
    assert not np.array_equal(outs[0][1], fc0[0])          # the steps did move the parameters
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_old_load_order_ships_in_the_measurement_build_only():
    with pytest.raises(_lib.VmapStepError, match="measurement build only"):
        step.VmapStep(2, 12, 10, 32, device=DEV, tuning=OLD_ORDER)
