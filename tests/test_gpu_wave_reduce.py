"""GPU tier: the product's step_main_s32 sums the B_layer.weight gradient with the transposing butterfly of
vmap_amd/csrc/wave_reduce.h; the measurement build keeps the form it replaces - one full butterfly per value, the former source in
a template instantiation of its own - behind tuning.ws_flags bit 3.  Same sum tree per value, so loss, flags, renders and all 15 gradients must be the same BITS, on shapes whose
waves and 16-lane rows are only partly filled (tests/test_wave_reduce_sim.py runs the same shapes on the CPU executor)."""
import numpy as np
import pytest

from conftest import GRAD_KEYS, RENDER_KEYS
from test_gpu_parity import DEV, _run
from vmap_amd import _lib, step, synth

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 10), (2, 5, 10), (3, 13, 10), (2, 12, 10)]
PER_VALUE = {"ws_flags": 8}


@pytest.mark.parametrize("n,R,S", SHAPES, ids=lambda v: str(v))
def test_transposing_butterfly_gives_the_bits_of_the_per_value_form(n, R, S):
    fc, B, sc = synth.make_params(n, 32, scale=2.0, seed=300 + R)
    batch = synth.make_batch(n, R, S, seed=400 + R)
    c = dict(n=n, R=R, S=S, H=32, fc=fc, B=B, scale=sc, batch=batch)
    new = _run(c, op=step.VmapStep(n, R, S, 32, device=DEV))                 # the product library, automatic plan
    old = _run(c, tuning=PER_VALUE)                                          # refused by the product -> the measurement build
    assert np.isfinite(new["g_B"]).all() and np.abs(new["g_B"]).max() > 0
    assert new["loss"] == old["loss"] and np.array_equal(new["flags"], old["flags"])
    for k in RENDER_KEYS + ["var"] + GRAD_KEYS:
        assert np.array_equal(new[k], old[k]), k


def test_per_value_form_ships_in_the_measurement_build_only():
    with pytest.raises(_lib.VmapStepError, match="measurement build only"):
        step.VmapStep(2, 12, 10, 32, device=DEV, tuning=PER_VALUE)
