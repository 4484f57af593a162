"""Exposed-wait census of one kernel: tests/tools/wait_census.py <unit> <kernel> <b,b,...> [--csrc DIR] [-DFLAG ...]

Compiles vmap_amd/csrc/<unit>.hip (or DIR/<unit>.hip) to gfx950 device assembly with __graft_entry__.HIPCC_FLAGS and prints, for the
instantiation <kernel><b,b,...> (template arguments as 0 / 1), per barrier segment: every vector or scalar memory load and every
s_waitcnt that names vmcnt, each with its position (instruction index in the kernel / in the segment), the segment's instruction
count and its count of DPP instructions; then the kernel's register and scratch figures.

A wave of this project's one-wave-per-SIMD kernels issues in order, so a vmcnt wait the wave reaches while a round trip is still in
flight stalls everything behind it: the census shows which waits stand where.  census() is what tests/test_s32_wait_census.py asserts
on.  It reads loads, waits, DPP and barrier mnemonics only."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LOAD = re.compile(r"^(global_load|buffer_load|flat_load|scratch_load|s_load|s_buffer_load)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
DPP = re.compile(r"(_dpp\b|\bquad_perm:|\brow_(shl|shr|ror|bcast|mirror|half_mirror|share|xmask|newbcast):?|\bwave_(shl|shr|rol|ror):)")


def device_asm(unit, csrc=None, flags=()):
    """The unit's gfx950 assembly as text (the product's flags + `flags`)."""
    csrc = csrc or ge.CSRC
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, unit + ".s")
        subprocess.run([hipcc] + ge.HIPCC_FLAGS + list(flags) + ["-cuid=vmapstep_" + unit, "--cuda-device-only", "-S", "-I", csrc,
                        os.path.join(csrc, unit + ".hip"), "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(out) as fh:
            return fh.read()


def mangled(kernel, bools):
    """Itanium name fragment of kernel<bools...> (a function template of boolean parameters in some namespace)."""
    return f"{len(kernel)}{kernel}I" + "".join(f"Lb{int(b)}E" for b in bools) + "EE"


def census(asm, kernel, bools):
    """{"name", "segments": [{"n", "dpp", "first_dpp", "events": [(pos, pos_in_segment, kind, text)]}], "meta": {...}} of one kernel.
    kind: "load" | "dma" (global_load_lds_*) | "wait" (s_waitcnt naming vmcnt; text holds the whole instruction)."""
    frag = mangled(kernel, bools)
    lines = asm.splitlines()
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(frag) + r"\w*:", l)), None)
    if start is None:
        raise KeyError(f"no kernel {kernel}<{','.join(str(int(b)) for b in bools)}> ({frag}) in the assembly")
    name = lines[start].split(":")[0]
    segs = [{"n": 0, "dpp": 0, "first_dpp": None, "events": []}]
    pos = 0
    end = start
    for end in range(start + 1, len(lines)):
        l = lines[end].split(";")[0].strip()
        if not l or l.startswith(".") or l.endswith(":"):
            if l.startswith(".Lfunc_end"):
                break
            continue
        mnem = l.split()[0]
        seg = segs[-1]
        if mnem == "s_barrier":
            seg["barrier_at"] = pos
            segs.append({"n": 0, "dpp": 0, "first_dpp": None, "events": []})
        elif LOAD.match(mnem):
            seg["events"].append((pos, seg["n"], "dma" if mnem.startswith("global_load_lds") else "load", l))
        elif mnem == "s_waitcnt" and VMCNT.search(l):
            seg["events"].append((pos, seg["n"], "wait", l))
        elif DPP.search(l):
            seg["dpp"] += 1
            if seg["first_dpp"] is None:
                seg["first_dpp"] = seg["n"]
        if mnem != "s_barrier":
            seg["n"] += 1
        pos += 1
    meta = {}
    for l in lines[end:end + 400]:          # the "Kernel info" comment block behind the kernel
        if re.match(r"^_Z\w+:", l):
            break
        m = re.match(r"^;\s*(ScratchSize|NumVgprs|NumAgprs|TotalNumVgprs|NumSgprs|Occupancy|LDSByteSize):\s*(\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
    return {"name": name, "instructions": pos, "segments": segs, "meta": meta}


def vmcnt_of(text):
    return int(VMCNT.search(text).group(1))


def render(c):
    out = [f"{c['name']}: {c['instructions']} instructions, {len(c['segments'])} barrier segments; " +
           ", ".join(f"{k} {v}" for k, v in sorted(c["meta"].items()))]
    for i, s in enumerate(c["segments"]):
        out.append(f"segment {i}: {s['n']} instructions, {s['dpp']} DPP" + (f" (first at +{s['first_dpp']})" if s["dpp"] else ""))
        ev, j = s["events"], 0
        while j < len(ev):
            pos, rel, kind, text = ev[j]
            k = j + 1
            while kind != "wait" and k < len(ev) and ev[k][2] == kind and ev[k][3].split()[0] == text.split()[0]:
                k += 1           # a run of one load mnemonic is one line
            out.append(f"  {pos:6d} +{rel:<5d} {text}" if k == j + 1 else f"  {pos:6d} +{rel:<5d} {k - j} x {text.split()[0]} .. +{ev[k - 1][1]}")
            j = k
    return "\n".join(out)


def main():
    args = sys.argv[1:]
    csrc = None
    if "--csrc" in args:
        i = args.index("--csrc")
        csrc = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    flags = [a for a in args if a.startswith("-D")]
    unit, kernel, bools = [a for a in args if not a.startswith("-D")][:3]
    print(render(census(device_asm(unit, csrc, flags), kernel, [int(b) for b in bools.split(",")])))


if __name__ == "__main__":
    main()
