"""CPU tier (needs hipcc, ~30 s): the backward of the shipped step_main_s32, read off its gfx950 assembly (tests/tools/gap_census.py).
One wave per SIMD issues in order, so VALU work hides behind a matrix instruction only where the two are interleaved in the instruction
stream - and the compiler places an untied result at its use, wherever the source formed it.  Pinned here, per barrier segment of the
backward (units 0..11 = the twelve segments behind the compositing's closing barrier, unit 12 = the B_layer unit behind them):

  * the mask / split chunks of mid2 and mid1 (units 3 and 5) stand behind the matrix instructions of their weight-gradient + bias chain:
    the source spreads 8 chunks over the chain's 10 slots (slots 0 and 5 get none), the parent commit had 1 slot of 10 filled;
  * the d(projection) multiply-adds stand in the units the source forms them in (1, 2 and the three in_layer blocks): 16 + 6 + 16 + 16 + 12
    = 66, every one the source places there - the parent had 0 (all 66 in the B_layer unit, which has no matrix instruction);
  * 18 of the 28 on-pipe transposes convert their result tile behind a long s_nop (the parent: 21).  Alternating the planes between two
    result tiles brought this to 0 and was measured SLOWER (sum of the phase stamps 43593 against 43258 clocks: tied to its unit, a
    transpose no longer overlaps the next unit's d-prop chain, which is what the compiler does with 10 of the planes on its own); it was
    not kept, so the count stays pinned where it is: it must not grow.  Every remaining site, by unit, in profiles/s32_backward_census.txt;
  * no scratch, and no more v_accvgpr_* moves than the parent's 247.

Reads mnemonics and the register operands of matrix instructions, conversions and s_nop only.  profiles/s32_backward_census.txt holds the
parent's and this commit's census."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc is missing")

PARENT_ACCVGPR = 247
DPROJ_FMA = {1: 16, 2: 6, 7: 16, 9: 16, 11: 12}        # unit: the products the source forms behind that unit's weight-gradient chain
LONG_NOP_SITES = 18                                     # reached (the parent: 21); the two-tile transposes that remove them were slower


@pytest.fixture(scope="module")
def cen():
    import gap_census
    import wait_census
    c = gap_census.census(wait_census.device_asm("k_s32"))
    print(gap_census.render(c, "step_main_s32<1,0,0,1,0,0,0>"))
    return c


def test_the_backward_is_thirteen_units(cen):
    assert len(cen["units"]) == 13
    assert all(u["mfma"] >= 12 for u in cen["units"][:12]) and cen["units"][12]["mfma"] == 0
    assert cen["mfma"] == 344 and cen["barriers"] == 18


@pytest.mark.parametrize("unit", [3, 5])
def test_mid_units_keep_their_chunks_in_the_chain(cen, unit):
    import gap_census
    u = cen["units"][unit]
    g = gap_census.db_chain_gaps(u)
    assert g is not None, u["mfma_ops"]
    print(f"unit {unit}: VALU behind the ten matrix instructions of mm_dw_il<true>:", g)
    assert len(g) == 10 and sum(1 for v in g if v > 0) >= 8


def test_dproj_products_stand_in_their_units(cen):
    got = {k: cen["units"][k]["fma"] for k in DPROJ_FMA}
    print("multiply(-add)s in units 1, 2, 7, 9, 11:", got, "- B_layer unit:", cen["units"][12]["fma"])
    assert got == DPROJ_FMA and sum(got.values()) == 66      # the source's 66, all of them
    for k in DPROJ_FMA:      # behind matrix instructions 0..3 of the unit's weight-gradient chain: its last six (unit 2: in front of F(d4)'s four)
        g = cen["units"][k]["gaps"]
        chain = g[-10:-4] if k == 2 else g[-6:]
        assert sum(1 for v in chain[:4] if v > 0) >= 3, g


def test_transposes_that_wait_out_the_pipe_did_not_grow(cen):
    sites = [(u["name"], u["nops"]) for u in cen["units"] if u["nops"]]
    print("long s_nop between a matrix instruction and a conversion of its result:", cen["nop_sites"], sites)
    assert cen["nop_sites"] <= LONG_NOP_SITES


def test_no_scratch(cen):
    assert cen["meta"]["ScratchSize"] == 0


def test_accvgpr_moves_did_not_grow(cen):
    print("v_accvgpr_* moves:", cen["accvgpr"])
    assert cen["accvgpr"] <= PARENT_ACCVGPR
