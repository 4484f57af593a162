"""Gap census of the backward of step_main_s32: tests/tools/gap_census.py [--csrc DIR] [-DFLAG ...]

Compiles vmap_amd/csrc/k_s32.hip (or DIR/k_s32.hip) to gfx950 device assembly with the product's flags and prints, for the shipped
instantiation and per barrier segment of its backward: the VALU instructions that stand behind each matrix instruction (the "gaps" of
the hand-interleaved chains), the multiply-adds, the conversions, and every long s_nop that stands between a matrix instruction and a
conversion of its result.  One wave per SIMD issues in order, so VALU work is free only where it stands between matrix instructions
in the instruction stream: the census shows what of the source's interleaving is in the code the GPU runs.

The backward's units 0..11 are the twelve segments behind the compositing's closing barrier (the first segment behind the forward that
holds matrix instructions again); the B_layer unit is the segment after them.  census() is what tests/test_s32_backward_census.py
asserts on.  It reads mnemonics and register operands of the matrix instructions, conversions and s_nop only."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wait_census  # noqa: E402

# step_main_s32<BWD, MULTI, STAMPS, W3, B6, PV, OL>: training, one pass per workgroup, float32 weights - what the headline step launches
SHIPPED = (1, 0, 0, 1, 0, 0, 0)
CVT = "v_cvt_pk_bf16_f32"
FMA = ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32", "v_mul_f32", "v_pk_mul_f32")
UNIT_NAMES = ["unit 0: colour x h4", "unit 1: colour x e2[0..15]", "unit 2: colour x e2[16..23]", "unit 3: mid2", "unit 4: cat x h2",
              "unit 5: mid1", "unit 6: cat x e1 block 0", "unit 7: in x e1 block 0", "unit 8: cat x e1 block 1", "unit 9: in x e1 block 1",
              "unit 10: cat x e1 block 2", "unit 11: in x e1 block 2", "unit 12: B_layer"]


def is_mfma(m):
    return m.startswith("v_mfma")


def is_valu(m):
    return m.startswith("v_") and not m.startswith(("v_mfma", "v_accvgpr", "v_nop"))


def _regs(op):
    """register numbers an operand such as v[12:27], a5 or v7 names (with its file letter)"""
    m = re.match(r"^([va])\[(\d+):(\d+)\]", op)
    if m:
        return {(m.group(1), r) for r in range(int(m.group(2)), int(m.group(3)) + 1)}
    m = re.match(r"^([va])(\d+)\b", op)
    return {(m.group(1), int(m.group(2)))} if m else set()


def instructions(asm, kernel="step_main_s32", bools=SHIPPED):
    """[(mnemonic, [operands])] of one instantiation"""
    frag = wait_census.mangled(kernel, bools)
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(frag) + r"\w*:", l))
    out = []
    for l in lines[start + 1:]:
        t = l.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            break
        if t and not t.startswith(".") and not t.endswith(":"):
            parts = t.split(None, 1)
            out.append((parts[0], [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []))
    return out


def segments(ins):
    segs, cur = [], []
    for i in ins:
        if i[0] == "s_barrier":
            segs.append(cur)
            cur = []
        else:
            cur.append(i)
    segs.append(cur)
    return segs


def backward_units(segs):
    """the thirteen segments of the backward: the last 13 segments that end at a barrier, in front of the pass's tail (the segment
    behind the backward's last barrier finishes the last block; the one behind the closing barrier writes the small vectors)"""
    with_mfma = [k for k, s in enumerate(segs) if any(is_mfma(m) for m, _ in s)]
    last = with_mfma[-1]            # unit 11: the last segment with matrix instructions
    return segs[last - 11:last + 2]


def gaps(seg):
    """VALU instructions behind each matrix instruction of a segment (up to the next one, or the segment's end)"""
    idx = [i for i, (m, _) in enumerate(seg) if is_mfma(m)]
    return [sum(1 for m, _ in seg[a + 1:b] if is_valu(m)) for a, b in zip(idx, idx[1:] + [len(seg)])]


def nop_sites(seg):
    """[(index in the segment, nop length)] of every s_nop >= 8 that stands directly behind a matrix instruction and directly in
    front of a conversion that reads that instruction's result"""
    out = []
    for i, (m, ops) in enumerate(seg):
        if m != "s_nop" or i == 0 or i + 1 >= len(seg):
            continue
        n = int(ops[0], 0)
        pm, pops = seg[i - 1]
        nm, nops = seg[i + 1]
        if n >= 8 and is_mfma(pm) and nm == CVT and (_regs(pops[0]) & (_regs(nops[1]) | _regs(nops[2]))):
            out.append((i, n))
    return out


def census(asm):
    ins = instructions(asm)
    segs = segments(ins)
    units = backward_units(segs)
    meta = wait_census.census(asm, "step_main_s32", SHIPPED)["meta"]
    rows = []
    for k, s in enumerate(units):
        g = gaps(s)
        idx = [i for i, (m, _) in enumerate(s) if is_mfma(m)]
        rows.append({"name": UNIT_NAMES[k], "n": len(s), "mfma": len(g), "gaps": g, "lead": idx[0] if idx else len(s),
                     "fma": sum(1 for m, _ in s if m.startswith(FMA)), "cvt": sum(1 for m, _ in s if m == CVT),
                     "accvgpr": sum(1 for m, _ in s if m.startswith("v_accvgpr")), "nops": nop_sites(s),
                     "mfma_ops": [s[i][1] for i in idx]})
    return {"instructions": len(ins), "mfma": sum(1 for m, _ in ins if is_mfma(m)), "barriers": len(segs) - 1,
            "accvgpr": sum(1 for m, _ in ins if m.startswith("v_accvgpr")), "meta": meta, "units": rows,
            "nop_sites": sum(len(nop_sites(s)) for s in segs)}


def db_chain_gaps(unit):
    """the gaps behind the ten matrix instructions of a mid unit's mm_dw_il<true> chain: the ones-column bias sums are the run of four
    matrix instructions that share one B operand (the ones) and one result tile, the first of them with C = 0; the six in front of
    them are the weight-gradient products.  None if the unit has no such run."""
    ops = unit["mfma_ops"]
    for i in range(6, len(ops) - 3):
        run = ops[i:i + 4]
        if all(o[2] == run[0][2] and o[0] == run[0][0] for o in run) and run[0][3] == "0" and all(o[3] == o[0] for o in run[1:]):
            return unit["gaps"][i - 6:i + 4]
    return None


def render(c, title):
    out = [f"{title}: {c['instructions']} instructions, {c['mfma']} matrix instructions, {c['barriers']} barriers, "
           f"{c['accvgpr']} v_accvgpr_* moves, {c['nop_sites']} long s_nop between a matrix instruction and a conversion of its result; " +
           ", ".join(f"{k} {v}" for k, v in sorted(c["meta"].items()))]
    for u in c["units"]:
        out.append(f"  {u['name']}: {u['n']} instructions, {u['lead']} in front of the first matrix instruction, {u['mfma']} matrix, "
                   f"{u['fma']} multiply(-add)s, {u['cvt']} conversions, {u['accvgpr']} accvgpr moves, {len(u['nops'])} long s_nop")
        out.append(f"    VALU behind each matrix instruction: {u['gaps']}")
    return "\n".join(out)


def main():
    args = sys.argv[1:]
    csrc = None
    if "--csrc" in args:
        i = args.index("--csrc")
        csrc = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    print(render(census(wait_census.device_asm("k_s32", csrc, [a for a in args if a.startswith("-D")])), "step_main_s32<1,0,0,1,0,0,0>"))


if __name__ == "__main__":
    main()
