"""GPU tier: step_main_s32 splits the encoding planes of e1[24..47] and e2 under the in_layer and mid1 matrix chains and forms the
backward's cos * pi * 2^f factors under the cat / mid2 / colour chains, instead of in front of the first chain; the measurement build keeps
the former order - the former source in a template instantiation of its own - behind tuning.ws_flags bit 5.  Every value is computed
by the same operations on the same operands, so loss, flags, renders, var and all 15 gradients of the PRODUCT must be the same BYTES as
the former order's, on shapes with one ray (most lanes padding), a partial last tile, a nearly empty second ray group, an exactly full
group, many objects, the longest ray of the 16-lane compositing, bf16 weights and the six-product backward."""
import numpy as np
import pytest
import torch

from conftest import AB_LIBRARY, GRAD_KEYS, RENDER_KEYS
from test_gpu_parity import DEV, _run
from vmap_amd import _lib, step, synth

pytestmark = pytest.mark.gpu

FORMER = {"ws_flags": 32}
# (n, R, S, weights, tuning)
SHAPES = [(1, 1, 10, "f32", {}), (2, 5, 10, "f32", {}), (3, 13, 10, "f32", {}), (2, 12, 10, "f32", {}), (40, 24, 10, "f32", {}),
          (2, 3, 16, "f32", {}), (2, 12, 10, "bf16", {}), (2, 12, 10, "f32", {"kernel": _lib.KERNEL_S32_BWD6})]


def _tobytes(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("n,R,S,weights,tuning", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_product_gives_the_bytes_of_the_former_order(n, R, S, weights, tuning):
    fc, B, sc = synth.make_params(n, 32, scale=2.0, seed=700 + R)
    batch = synth.make_batch(n, R, S, seed=800 + R + S)
    c = dict(n=n, R=R, S=S, H=32, fc=fc, B=B, scale=sc, batch=batch)
    new = _run(c, op=step.VmapStep(n, R, S, 32, device=DEV, weights=weights, tuning=dict(tuning) or None))
    old = _run(c, op=step.VmapStep(n, R, S, 32, device=DEV, weights=weights, tuning={**tuning, **FORMER}, library=AB_LIBRARY))
    assert np.isfinite(new["g_B"]).all() and np.abs(new["g_B"]).max() > 0
    assert np.float32(new["loss"]).tobytes() == np.float32(old["loss"]).tobytes()
    assert _tobytes(new["flags"]) == _tobytes(old["flags"])
    for k in RENDER_KEYS + ["var"] + GRAD_KEYS:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and _tobytes(new[k]) == _tobytes(old[k]), k


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


def test_former_order_ships_in_the_measurement_build_only():
    with pytest.raises(_lib.VmapStepError, match="measurement build only"):
        step.VmapStep(2, 12, 10, 32, device=DEV, tuning=FORMER)
