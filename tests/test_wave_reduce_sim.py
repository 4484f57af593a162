"""CPU tier: step_main_s32 with the transposing butterfly of vmap_amd/csrc/wave_reduce.h (the B_layer.weight gradient: sixteen half-wave
sums at once, each left on one lane) on the SIMT executor, on shapes whose waves and 16-lane rows are only partly filled - one ray
(10 of a wave's 32 points), 50 and 130 points (a wave with 18 / 2 points: a full and a part-filled row / a single quad), 120 points
(24 in the last wave).  Padding lanes contribute zeros to every sum; a partner, key or register-slot mistake in the butterfly moves
B_layer.weight's gradient (and nothing else) away from the oracle.  Bars: those of tests/test_kernel_sim.py."""
import numpy as np
import pytest

import simlib
from conftest import GRAD_KEYS, RENDER_KEYS, relerr
from oracle import vmap_oracle as vo
from vmap_amd import synth

SHAPES = [(1, 1, 10), (2, 5, 10), (3, 13, 10), (2, 12, 10)]


@pytest.mark.parametrize("n,R,S", SHAPES, ids=lambda v: str(v))
def test_sim_split_kernel_on_part_filled_waves_and_rows(n, R, S):
    fc, B, sc = synth.make_params(n, 32, scale=2.0, seed=300 + R)
    batch = synth.make_batch(n, R, S, seed=400 + R)
    o = vo.training_step(fc, B, sc, batch, dtype=np.float32)
    s = simlib.sim_step(fc, B, sc, batch, split=True)
    assert abs(s["loss"] - o["loss"]) <= 2e-5 * abs(o["loss"])
    for k in RENDER_KEYS:
        assert relerr(s[k], o[k]) < 2e-5, k
    for k in GRAD_KEYS:
        assert not np.isnan(s[k]).any(), k
        assert relerr(s[k], o[k]) < 1e-4, k
    assert s["flags"][:3].tolist() == [int(x) for x in o["drop"]]
