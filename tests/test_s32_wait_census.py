"""CPU tier (needs hipcc, ~30 s): where the shipped step_main_s32 waits for memory, read off its gfx950 assembly by
tests/tools/wait_census.py.  One wave per SIMD issues in order, so a vmcnt wait reached while a round trip is in flight stalls
everything behind it - and the compiler flushes vmcnt to ZERO at any wait while an LDS-DMA is pending.  Pinned here: the image copy
stays in flight under the encoding, the compositing opens without a load or a memory wait, the forward's loads are requested at its
head.  Reads loads, waits, DPP and barrier mnemonics only."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc is missing")

# step_main_s32<BWD, MULTI, STAMPS, W3, B6, PV, OL>: training, one pass per workgroup, float32 weights - what the headline step launches
SHIPPED = (1, 0, 0, 1, 0, 0, 0)


@pytest.fixture(scope="module")
def census():
    import wait_census
    c = wait_census.census(wait_census.device_asm("k_s32"), "step_main_s32", SHIPPED)
    print(wait_census.render(c))
    return c


def _segments(c):
    """(copy, forward, compositing): the segment holding the LDS-DMA and the two behind it."""
    segs = c["segments"]
    i = next(k for k, s in enumerate(segs) if any(e[2] == "dma" for e in s["events"]))
    assert [k for k, s in enumerate(segs) if any(e[2] == "dma" for e in s["events"])] == [i]
    return segs[i], segs[i + 1], segs[i + 2]


def test_image_copy_stays_in_flight_under_the_encoding(census):
    import wait_census
    seg = _segments(census)[0]
    ev = seg["events"]
    dma = [e for e in ev if e[2] == "dma"]
    assert len(dma) == 20
    waits = [e for e in ev if e[2] == "wait"]
    drain = waits[-1]                                            # the closing drain: the last wait, in front of the barrier (only address
    assert drain[1] > dma[-1][1] and seg["n"] - drain[1] <= 40, drain      # arithmetic of the loads behind the barrier may stand between)
    assert seg["n"] - dma[-1][1] > 500                           # the encoding stands behind the copy, not in front of it
    for e in waits[:-1]:
        issued = sum(1 for d in dma if d[1] < e[1])
        assert issued == 0 or wait_census.vmcnt_of(e[3]) >= issued, (e, issued)


def test_compositing_opens_without_a_load_or_a_memory_wait(census):
    seg = _segments(census)[2]
    assert seg["dpp"] >= 100, seg["dpp"]                         # it IS the compositing: the scans are DPP
    early = [e for e in seg["events"] if e[1] < seg["first_dpp"] and (e[2] == "wait" or e[3].startswith(("global_load", "buffer_load", "flat_load")))]
    assert not early, early


def test_forward_requests_its_loads_at_its_head(census):
    seg = _segments(census)[1]
    loads = [e for e in seg["events"] if e[3].startswith("global_load")]
    assert len(loads) >= 9, loads                                # two masks, depth, three colours, the switches, the counts, z
    late = [e for e in loads if e[1] >= seg["n"] - 100]
    assert not late, late


def test_registers_and_scratch(census):
    m = census["meta"]
    assert m["ScratchSize"] == 0
    assert m["TotalNumVgprs"] <= 512
