"""CPU tier: the step plan (vmap_amd/csrc/step_plan.h) - kernel family, rounds, workspace sections - compiled twice, by hipcc into
the two libraries and by the host compiler into the CPU executor, must be one plan; the plan keeps what its comments promise; and
it is the plan the library made before the header existed (tests/step_plan_table.txt, recorded from that library).  No device."""
import ctypes
import importlib.util
import itertools
import os

import pytest

import simlib
from conftest import AB_LIBRARY, ROOT
from vmap_amd import _lib, layout

_spec = importlib.util.spec_from_file_location("step_plan_dump", os.path.join(ROOT, "tests", "tools", "step_plan_dump.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)

KERNEL_NAMES = {"h32": "step_main_h32", "s32": "step_main_s32", "s32_bwd6": "step_main_s32<bwd6>", "gen": "step_main_gen",
                "wide": "step_main_wide<4>", "ws": "step_main_ws<%d>", "wp": "step_main_wp<%d>"}
OFFSETS = ("off_ploss", "off_imgtab", "off_tab_wt", "off_row_tab", "off_pgrad", "off_wimg", "off_scratch", "off_flags", "off_stats", "total")


def shape_of(e):
    """-> (Shape, the Tuning it points to: keep it alive)"""
    sh = _lib.Shape(*e[:5])
    t = _lib.Tuning(*e[5]) if e[5] is not None else None
    if t is not None:
        sh.tuning = ctypes.pointer(t)
    return sh, t


def executor_answer(e, measurement_build):
    """The executor's compilation of the plan for a grid entry, in the form step_plan_dump.Asker gives the library's: every field
    vmapstep_describe_plan, vmapstep_workspace_bytes and vmapstep_workspace_counts_offset expose."""
    sh, _keep = shape_of(e)
    rc, msg, p = simlib.step_plan(sh, e[6], measurement_build)
    if rc:
        return (rc, msg), None
    nb, fam = e[3] // 32, p["family"]
    name = KERNEL_NAMES[fam] % nb if "%" in KERNEL_NAMES[fam] else KERNEL_NAMES[fam]
    waves = (8 if nb > 4 else 4) if fam == "ws" else 2 * nb if fam == "wp" else 4
    return (0, "", name, p["G"], p["NG"], p["NW"], p["tiles"] if fam == "ws" else 0, waves, int(p["NG"] == p["NW"]), p["total"], p["off_stats"]), p


def grid_of(hidden):
    return dict(dump.FULL, hidden=(hidden,))


@pytest.mark.parametrize("hidden", dump.HIDDEN)
@pytest.mark.parametrize("build", ["product", "measurement"])
def test_both_compilations_make_the_same_plan(build, hidden):
    """The full grid of the plan's inputs (tests/tools/step_plan_dump.py: shapes at and around every threshold of the rules, every
    tuning value on its own, invalid values of each), one width per case: status, message and every exposed field are equal between
    the library (hipcc) and the executor (host compiler) - the product library against measurement_build = false, the measurement
    build against true."""
    ask = dump.Asker(None if build == "product" else AB_LIBRARY)
    for e in dump.entries(grid_of(hidden)):
        got, _ = executor_answer(e, build == "measurement")
        assert got == ask(e), e


def need(fam, e, p):
    """Bytes each section must hold, in OFFSETS' order, as far as the argument blocks' comments define them (StepArgs, FinalizeArgs:
    [n][NW][4] loss partials, [PP] / [PR] tables, [n][NW][PR] gradient rows, [kMaxFrameSteps][4] flags, [steps][n][4] counts); the
    image and the scratch are the kernel headers' business: something, where the family has them"""
    n, hidden, max_steps = e[0], e[3], e[6]
    PP = (layout.param_count(hidden) + 63) // 64 * 64
    blocks = fam in ("ws", "wp")
    assert p["PR"] == PP or (blocks and p["PR"] > PP and p["PR"] % 64 == 0)
    return (16 * n * p["NW"], 4 * PP if blocks or hidden == 32 else 0, 4 * PP if blocks else 0, 4 * p["PR"] if blocks else 0,
            4 * n * p["NW"] * p["PR"], 4 * n, 1 if hidden != 32 else 0, 16 * 256, 16 * max_steps * n)


@pytest.mark.parametrize("hidden", [h for h in dump.HIDDEN if 32 <= h <= 256 and h % 32 == 0])
def test_plan_invariants(hidden):
    """What the comments of step_plan.h promise, at every grid entry the measurement build's plan accepts (it accepts what the
    product's does, and the A/B forms): sections 256-byte aligned, in order, each at least as large as its contents, the last ending
    at the total; no offset depends on the step count; 1 <= NW <= NG = ceil(R / G); a round's points within the family's capacity;
    step_main_ws / _wp with automatic workgroups: rounds per workgroup differ by at most one, and no fewer workgroups would do for
    the same busiest workgroup ("spread the rounds evenly - fewer partial-gradient rows": per = ceil(NG / NW) rounds need
    ceil(NG / per) workgroups, no more)."""
    g = grid_of(hidden)
    accepted = 0
    for head in itertools.product(g["n_obj"], g["rays"], g["samples"], g["hidden"], g["weights"], g["tunings"]):
        offsets = set()
        for max_steps in g["max_steps"]:
            e = head + (max_steps,)
            got, p = executor_answer(e, True)
            if p is None:
                continue
            accepted += 1
            n, R, S, fam = e[0], e[1], e[2], p["family"]
            offs = [p[k] for k in OFFSETS]
            assert offs[0] == 0 and all(o % 256 == 0 for o in offs) and offs == sorted(offs), (e, offs)
            for k, lo, hi, size in zip(OFFSETS, offs, offs[1:], need(fam, e, p)):
                assert hi - lo >= size and (hi - lo == 0) == (size == 0), (e, k)
            assert offs[-1] - offs[-2] == (16 * max_steps * n + 255) // 256 * 256, e
            offsets.add(tuple(offs[:-1]))
            assert 1 <= p["NW"] <= p["NG"] == -(-R // p["G"]), e
            assert p["G"] * S <= {"ws": 32 * p["tiles"], "wp": 64, "wide": 32}.get(fam, 128), e
            assert (fam in ("h32", "s32", "s32_bwd6")) == (hidden == 32), e
            if fam in ("ws", "wp") and (e[5] is None or e[5][0] <= 0):
                per = [len(range(w, p["NG"], p["NW"])) for w in range(p["NW"])]       # workgroup w takes rounds w, w + NW, ...
                assert max(per) - min(per) <= 1 and p["NW"] == -(-p["NG"] // max(per)), e
        assert len(offsets) <= 1, head
    assert accepted > 1000


def test_plans_are_the_recorded_ones():
    """tests/step_plan_table.txt: plan lines of a reduced grid (step_plan_dump.py --reduced) recorded from the library as it was
    before the plan moved into step_plan.h.  The library and the executor reproduce them."""
    with open(os.path.join(ROOT, "tests", "step_plan_table.txt")) as fh:
        recorded = fh.read().splitlines()
    ask = dump.Asker(None)
    entries = list(dump.entries(dump.REDUCED, dump.REDUCED_EXTRA))
    assert len(entries) == len(recorded) > 250
    for e, want in zip(entries, recorded):
        assert dump.line(e, ask(e)) == want
        assert dump.line(e, executor_answer(e, False)[0]) == want
