"""CPU tier (needs hipcc, ~30 s): the front of the shipped step_main_s32, read off its gfx950 assembly.  One wave per SIMD issues in
order, so VALU work hides behind a matrix instruction only where the two are interleaved in the instruction stream.  Pinned here: of the
encoding's 36 register pairs only the 12 that the in_layer chain reads first (16-deep steps 0..2) are split into bf16 planes in front of
that chain - the other 24 are split behind its matrix instructions and mid1's - and the kernel does not spill.  Reads mnemonics only."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc is missing")

# step_main_s32<BWD, MULTI, STAMPS, W3, B6, PV, OL>: training, one pass per workgroup, float32 weights - what the headline step launches
SHIPPED = (1, 0, 0, 1, 0, 0, 0)
CVT = "v_cvt_pk_bf16_f32"
# Conversions allowed in the segment that ends at the image barrier: 12 pairs x 3 planes of e1[0..23], + what the parent commit has
# there outside split_planes.  The parent's census (tests/tools/wait_census.py layout, counted per barrier segment) has NO bf16
# conversion in that segment outside split_planes: everything in front of the barrier is float32 arithmetic (projection, sincos,
# double-angle recurrence), the first bf16 operands of the kernel are the encoding's planes.  (The parent's compiler placed even the
# 108 conversions of split_planes behind the barrier, in front of the first matrix instruction: its segment held 0.)  So: 36 + 0.
FRONT_CVT_BOUND = 12 * 3 + 0


def _instructions(asm, kernel, bools):
    import wait_census
    frag = wait_census.mangled(kernel, bools)
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(frag) + r"\w*:", l))
    out = []
    for l in lines[start + 1:]:
        t = l.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            break
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append(t.split()[0])
    return out


@pytest.fixture(scope="module")
def front():
    """(mnemonics of the segment that ends at the image barrier, mnemonics of the segment behind it, kernel meta)"""
    import wait_census
    asm = wait_census.device_asm("k_s32")
    meta = wait_census.census(asm, "step_main_s32", SHIPPED)["meta"]
    segs, cur = [], []
    for m in _instructions(asm, "step_main_s32", SHIPPED):
        if m == "s_barrier":
            segs.append(cur)
            cur = []
        else:
            cur.append(m)
    segs.append(cur)
    copy = [k for k, s in enumerate(segs) if any(m.startswith("global_load_lds") for m in s)]
    assert len(copy) == 1, copy                                   # the image copy: the segment's closing barrier is the image barrier
    return segs[copy[0]], segs[copy[0] + 1], meta


def _is_valu(m):
    return m.startswith("v_") and not m.startswith(("v_mfma", "v_accvgpr", "v_nop"))


def test_only_the_first_twelve_pairs_are_split_in_front_of_the_image_barrier(front):
    seg, fwd, _ = front
    n = sum(1 for m in seg if m == CVT)
    print("conversions in the segment that ends at the image barrier:", n)
    assert n <= FRONT_CVT_BOUND
    # the compiler may place the front's conversions on either side of the barrier; what the wave's chain sees is everything in front of
    # the first matrix instruction.  Same bound (the parent had all 36 pairs x 3 planes there).
    first = next(i for i, m in enumerate(fwd) if m.startswith("v_mfma"))
    n_front = n + sum(1 for m in fwd[:first] if m == CVT)
    print("conversions in front of the first matrix instruction:", n_front, "- instructions between the barrier and it:", first)
    assert n_front <= FRONT_CVT_BOUND


def test_the_first_matrix_chain_carries_valu_work(front):
    _, fwd, _ = front
    idx = [i for i, m in enumerate(fwd) if m.startswith("v_mfma")]
    assert len(idx) > 36
    filled = [sum(1 for m in fwd[a + 1:b] if _is_valu(m)) for a, b in zip(idx[:36], idx[1:37])]
    print("VALU instructions behind each of the first 36 matrix instructions:", filled)
    assert sum(1 for v in filled if v > 0) >= 30


def test_no_scratch(front):
    assert front[2]["ScratchSize"] == 0
