"""CPU tier of the instance tracker: csrc/track_rules.h - compiled into the host program tests/tools/track_rules_host.cpp with the
address and undefined-behaviour sanitizers - against the numpy checker (tests/track_oracle.py) answer for answer; the checker on the
sequences of tests/track_cases.py with hand-made boxes (the numpy backend of the box search), so that every case is known to produce
the status it is named for; and the argument checks of vmapstep_track_* (no device is touched).  Neither Open3D nor OpenCV is
involved anywhere: what is pinned is the contract of include/vmapstep.h."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import track_cases as tc
import track_oracle as to
from conftest import ROOT
from vmap_amd import _lib


# ---- csrc/track_rules.h on the host -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """A stand-alone program with its own main, built with -fsanitize=address,undefined: any out-of-bounds access or undefined
    arithmetic in the rules aborts it."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("track_host") / "track_rules_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vmap_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "track_rules_host.cpp"), "-o", exe], check=True)
    return exe


def compare(exe, tmp_path, lines, want):
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(lines) + "\n")
    got = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    asked = [l for l in lines if l[0] != "B"]
    assert len(got) == len(want) == len(asked)
    bad = [(l, g, w) for l, g, w in zip(asked, got, want) if g != w]
    assert not bad, bad[:5]


def test_host_ratio_test_equals_the_oracle_at_the_threshold_and_near_2_31(host_exe, tmp_path):
    """inside / valid against match_ratio exactly at, one below and one above the threshold, for small counts and for counts near 2^31,
    where both products leave 32 bits."""
    lines, want = [], []
    big = 2 ** 31 - 1
    for rq in (0, 1, 65536 // 4, 65536 // 2, 39322, 65535, 65536):
        for valid in (0, 1, 2, 10, 1000, 65536, 2 ** 30, big - 1, big):
            at = rq * valid // 65536                          # the largest inside that is not past the ratio when the product divides
            for inside in {0, max(at - 1, 0), at, min(at + 1, big), valid}:
                lines.append(f"M {inside} {valid} {rq}")
                want.append(str(int(inside * 65536 > rq * valid)))
                assert to.matches(inside, valid, rq) == (inside * 65536 > rq * valid)
    assert to.ratio_q(0.5) == 32768 and to.ratio_q(0.6) == 39322 and to.ratio_q(1.0) == 65536
    assert not to.matches((1 << 30) - 1, big - 1, 32768) and to.matches(1 << 30, big - 1, 32768) and not to.matches(5, 10, 32768) and to.matches(6, 10, 32768)
    assert "1" in want and "0" in want
    compare(host_exe, tmp_path, lines, want)


def test_host_decisions_equal_the_oracle_on_every_branch(host_exe, tmp_path):
    rng = np.random.default_rng(9)
    bg = [1, 3, -1]
    lines, want = [f"B {len(bg)} " + " ".join(map(str, bg))], []
    matched = set()
    for _ in range(4000):
        d = int(rng.choice([0, 1, 2, 40, 4095]))
        cls = int(rng.choice([-1, 1, 3, 7, 52]))
        min_pixels, min_points, rq = int(rng.choice([20, 2000])), int(rng.choice([0, 10])), int(rng.choice([0, 32768, 39322, 65536]))
        pixels = 0 if rng.random() < 0.05 else int(rng.choice([1, 500, 5000, 2 ** 31 - 1]))
        valid = int(rng.choice([0, 9, 11, pixels // 2, pixels]))
        eroded = int(rng.choice([0, 19, 20, 21, 1999, 2000, 2001, pixels]))
        eroded_valid = int(rng.choice([0, 9, 10, 11, min(eroded, valid)]))
        n = int(rng.choice([0, 1, 2, 5]))
        half = rq * valid // 65536
        inside = [int(rng.choice([0, max(half - 1, 0), half, min(half + 1, valid), valid])) for _ in range(n)]
        lines.append(f"R {d} {cls} {min_pixels} {min_points} {rq} {pixels} {valid} {eroded} {eroded_valid} {n} " + " ".join(map(str, inside)))
        st, j = to.decide(d, cls, pixels, valid, eroded, eroded_valid, inside, min_pixels, min_points, rq, bg)
        want.append(f"{st} {j}")
        if st == to.MERGED:
            matched.add(j)
            assert not any(to.matches(i, valid, rq) for i in inside[:j])
    assert {int(w.split()[0]) for w in want} == {to.ABSENT, to.NEW, to.MERGED, to.BACKGROUND, to.FEW_POINTS, to.SMALL}
    assert matched >= {0, 1, 2}                               # the first past the ratio, not only candidate 0
    # a later candidate with a higher ratio does not win; <= in both size tests
    for args, w in ((("1 7 20 10 32768 100 100 50 50 3", "40 60 100"), (to.MERGED, 1)), (("1 7 20 10 32768 100 100 20 50 1", "100"), (to.SMALL, -1)),
                    (("1 7 20 10 32768 100 100 21 10 1", "100"), (to.FEW_POINTS, -1)), (("1 7 20 10 32768 100 100 21 11 2", "50 50"), (to.NEW, -1)),
                    (("0 7 20 10 32768 100 100 50 50 1", "100"), (to.BACKGROUND, -1)), (("1 3 20 10 32768 100 100 50 50 1", "100"), (to.BACKGROUND, -1)),
                    (("1 7 20 10 32768 0 0 0 0 0", ""), (to.ABSENT, -1))):
        f = [int(x) for x in args[0].split()]
        assert to.decide(f[0], f[1], f[5], f[6], f[7], f[8], [int(x) for x in args[1].split()], f[2], f[3], f[4], bg) == w
        lines.append(f"R {args[0]} {args[1]}".rstrip())
        want.append(f"{w[0]} {w[1]}")
    for idv in (1, 7, 63):
        for st in range(9):
            for valid in (0, 1):
                for inside in (0, 1):
                    lines.append(f"L {idv} {st} {valid} {inside}")
                    want.append(str(to.label_of(idv, st, valid, inside)))
    for st in range(9):
        for flags in range(8):
            lines.append(f"E {st} {flags}")
            want.append(str(int(to.emits(st, flags))))
    compare(host_exe, tmp_path, lines, want)


# ---- the sequences through the checker, the boxes from the numpy backend of the search -----------------------------------------------

def oracle_tracker(**kw):
    s = dict(tc.SETTINGS, **kw)
    return to.Tracker(tc.W, tc.H, tc.INTRINSICS, s["depth_scale"], s["max_depth"], s["background"], s["match_ratio"], s["min_pixels"], s["min_points"],
                      s["erode_radius"], s["voxel_size"], 0, s["max_det"], s["max_ids"])


def register(table, trk, out):
    """What InstanceTracker does after a frame, with the numpy backend of the box search."""
    from vmap_amd import bounds, instances
    for i in out["new"] + out["merged"]:
        keys = trk.keys[(trk.keys >> 48) == i]
        box = bounds.oriented_bounds(to.fo.key_points(keys, trk.voxel), backend="numpy", min_extent=tc.SETTINGS["min_extent"])[0]
        assert box is not None
        table[i] = instances.box_row(box, 0.875 * trk.voxel)


def run(frames, **kw):
    trk = oracle_tracker(**kw)
    table = np.zeros((tc.SETTINGS["max_ids"], 16), np.float32)
    outs = []
    for rows, classes, depth, t_wc in frames:
        outs.append(trk.put(depth, rows, classes, t_wc, table))
        register(table, trk, outs[-1])
    return trk, table, outs


@pytest.fixture(scope="module")
def main_run():
    return run(tc.main_sequence())


def test_first_frame_yields_every_non_match_status(main_run):
    trk, _, (one, two, three) = main_run
    row = {name: d for d, name in enumerate(tc.ORDER_1, 1)}
    want = {0: to.BACKGROUND, row["A"]: to.NEW, row["B"]: to.NEW, row["C"]: to.NEW, row["BG"]: to.BACKGROUND, row["THIN"]: to.SMALL,
            row["FEW"]: to.FEW_POINTS, row["TINY"]: to.NEW_NO_BOX, row["D"]: to.NEW, row["E"]: to.NEW}
    assert one["status"] == want
    assert one["ids"] == {row[n]: i for n, i in tc.IDS.items()} and one["new"] == [1, 2, 3, 5, 6]       # id 4 was TINY's: a gap
    rows = {int(r[0]): r for r in one["rows"]}
    assert rows[row["TINY"]][3] == 4 and rows[row["FEW"]][8] == tc.SETTINGS["min_points"] and rows[row["THIN"]][7] == 0
    assert rows[row["A"]][7] == 12 * 14 and rows[row["A"]][5] == 14 * 16 - 1                      # one pixel beyond max_depth
    assert one["overflow"] == 0 and one["out_of_grid"] == 0 and len(one["pairs"]) == 0
    assert set(np.unique(one["labels"]).tolist()) == {0, 1, 2, 3, 5, 6} and set((trk.keys >> 48).tolist()) == {1, 2, 3, 5, 6, 7, 8}


def test_scrambled_rows_from_a_moved_pose_keep_their_ids(main_run):
    _, _, (one, two, three) = main_run
    row = {name: d for d, name in enumerate(tc.ORDER_2, 1)}
    assert two["ids"] == {row[n]: i for n, i in tc.IDS.items()} and not two["new"] and two["merged"] == [1, 2, 3, 5, 6]
    assert two["status"][row["BG"]] == to.BACKGROUND and two["status"][row["THIN"]] == to.SMALL and two["status"][row["FEW"]] == to.FEW_POINTS
    frame = tc.main_sequence()[1]
    for name, i in tc.IDS.items():
        own = two["labels"][frame[0] == row[name]]
        assert set(own.tolist()) == {i, -1}, name                 # its pixels carry both the id and -1
    # A and B share a class: each row has both as candidates, in ascending id
    assert [tuple(p[:2]) for p in two["pairs"] if p[0] == row["B"]] == [(row["B"], 1), (row["B"], 2)]


def test_labels_do_not_depend_on_the_numbering_of_the_rows(main_run):
    frames = tc.main_sequence()
    want = main_run[2][1]["labels"]
    rows, classes, depth, t_wc = frames[1]
    perm = np.array([0, 5, 3, 8, 1, 7, 2, 6, 4])                 # row d becomes row perm[d]
    classes2 = [0] * len(classes)
    for d, c in enumerate(classes):
        classes2[perm[d]] = c
    trk, table, _ = run(frames[:1])
    out = trk.put(depth, perm[rows], classes2, t_wc, table)
    assert np.array_equal(out["labels"], want) and out["ids"] == {int(perm[d]): i for d, i in main_run[2][1]["ids"].items()}


def test_third_frame_class_mismatch_below_threshold_and_shared_match(main_run):
    trk, _, (one, two, three) = main_run
    assert three["status"] == {0: to.BACKGROUND, 1: to.NEW, 2: to.NEW, 3: to.MERGED, 4: to.MERGED, 5: to.MERGED}
    assert three["ids"] == {1: 7, 2: 8, 3: 1, 4: 1, 5: 2} and three["new"] == [7, 8] and three["merged"] == [1, 2]
    pairs = {(int(d), int(i)): int(n) for d, i, n in three["pairs"]}
    assert not any(d == 1 for d, _ in pairs)                  # class 77 has no instance: no candidate, although C's box is there
    rows = {int(r[0]): r for r in three["rows"]}
    assert 0 < pairs[(2, 6)] * 2 <= rows[2][5]                # some of it inside E's box, not more than half
    assert pairs[(3, 1)] * 2 > rows[3][5] and pairs[(4, 1)] * 2 > rows[4][5] and pairs[(3, 2)] == 0
    assert trk.class_of == {1: 50, 2: 50, 3: 51, 5: 51, 6: 53, 7: 77, 8: 53} and trk.next_id == 9


def test_overlapping_candidates_the_lower_id_wins():
    trk, _, (one, two, three) = run(tc.overlap_sequence())
    assert one["ids"] == {1: 1} and two["status"][1] == to.NEW and two["ids"] == {1: 2}
    (d1, i1, n1), (d2, i2, n2) = three["pairs"].tolist()
    valid = int(three["rows"][1][5])
    assert (i1, i2) == (1, 2) and n2 > n1 and to.matches(n1, valid, trk.rq) and to.matches(n2, valid, trk.rq)
    assert three["status"][1] == to.MERGED and three["ids"] == {1: 1} and three["rows"][1][6] == n1


def test_overflow_sequence_offers_more_pairs_than_the_lds_table_holds():
    trk, _, (one, two, three) = run(tc.overflow_sequence(_lib.TRACK_PAIR_SLOTS))
    assert one["new"] == [1, 2, 3, 4, 5] and two["new"] == [6, 7, 8, 9, 10]
    tile = three["pairs"][three["pairs"][:, 0] <= 12]
    assert len(tile) == 120 > _lib.TRACK_PAIR_SLOTS
    late = tile[_lib.TRACK_PAIR_SLOTS + 4:]                   # past the table and its probes, in the order one wave meets them
    assert (late[:, 2] > 0).sum() >= 4
    assert set(three["status"].values()) == {to.BACKGROUND, to.SMALL}


def test_key_grid_edge_and_the_error_cases_through_the_oracle():
    frames = tc.main_sequence()
    rows, classes, depth, _ = frames[0]
    table = np.zeros((tc.SETTINGS["max_ids"], 16), np.float32)
    edge = 32768 * tc.SETTINGS["voxel_size"]
    e_rows, e_classes, e_depth = tc.edge_frame()
    near = oracle_tracker().put(e_depth, e_rows, e_classes, tc.pose(tx=edge - 0.3), table)
    assert near["out_of_grid"] > 0 and near["new"] == [1, 2, 3, 4, 5] and {int(k) >> 48 for k in near["frame_keys"]} == {1, 2, 3, 4, 5}
    ids = near["rows"][:, 3].tolist()                         # C and D are cut: fewer keys than their twins of the same size
    assert all(0 < (near["frame_keys"] >> 48 == i).sum() < (near["frame_keys"] >> 48 == 2).sum() for i in (3, 4)) and ids.count(0) == 4
    far = oracle_tracker().put(e_depth, e_rows, e_classes, tc.pose(tx=edge + 50.0), table)
    assert far["out_of_grid"] > 0 and len(far["frame_keys"]) == 0 and not far["new"]
    bad = rows.copy()
    bad[0, 0] = tc.SETTINGS["max_det"]
    assert oracle_tracker().put(depth, bad, classes, tc.pose(), table)["overflow"] == 1
    assert oracle_tracker().put(depth, rows, classes[:6], tc.pose(), table)["unnamed"] == [6, 7, 8, 9]
    assert oracle_tracker(max_ids=6).put(depth, rows, classes, tc.pose(), table)["full"]
    assert not oracle_tracker(max_ids=7).put(depth, rows, classes, tc.pose(), table)["full"]


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

def _cfg(width=75, height=53, max_det=32, max_pairs=256, max_ids=64, erode_radius=6, n_background=2, voxel_size=0.04, n_det=10, n_pairs=0, next_id=1,
         ratio_q=32768):
    bg = (ctypes.c_int32 * 64)(1, 3)
    pose = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    return _lib.TrackCfg(width, height, 0, 0, 1.0 / 1000.0, 8.0, 60.0, 60.0, 37.0, 26.0, pose, voxel_size, 0, 20, 10, erode_radius, max_det, max_pairs,
                         max_ids, n_det, n_pairs, next_id, ratio_q, n_background, bg)


def test_abi_refuses_bad_arguments_before_anything_is_enqueued():
    """One call per return code, none of which reads a pointer or touches a device: -1 for null or inconsistent arguments, -2 past a
    limit, -3 for a short or misaligned workspace - which is also as far as a well-formed call gets here."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    n = ctypes.c_size_t()
    ref = ctypes.byref
    assert lib.vmapstep_track_workspace_bytes(ref(_cfg()), ref(n)) == 0 and n.value >= 8 * 32 * 4 * 4 + 8 * 256 * 4 + 75 * 53
    need = n.value
    top = dict(max_det=4096, max_pairs=65536, max_ids=32767, width=4095, height=4095, erode_radius=8)
    assert lib.vmapstep_track_workspace_bytes(ref(_cfg(**top)), ref(n)) == 0 and n.value > need
    assert lib.vmapstep_track_workspace_bytes(ref(_cfg()), None) == -1 and lib.vmapstep_track_workspace_bytes(None, ref(n)) == -1
    limits = (dict(max_det=0), dict(max_det=4097), dict(max_pairs=0), dict(max_pairs=65537), dict(max_ids=1), dict(max_ids=32768), dict(erode_radius=-1),
              dict(erode_radius=9), dict(width=4096), dict(height=4096), dict(n_background=65), dict(n_pairs=257))
    for kw in limits:
        assert lib.vmapstep_track_workspace_bytes(ref(_cfg(**kw)), ref(n)) == -2 and b"track limits" in lib.vmapstep_last_error(), kw
    stats = lambda cfg, ws=need, depth=p, ident=p, wsp=p: lib.vmapstep_track_stats(cfg, depth, p, p, p, p, ident, p, wsp, ws, None)
    emit = lambda cfg, ws=need, keys=p, wsp=p: lib.vmapstep_track_emit(cfg, p, p, p, p, p, keys, p, wsp, ws, None)
    write = lambda cfg, labels=p: lib.vmapstep_track_write(cfg, p, p, p, p, p, labels, None)
    assert stats(None) == -1 and stats(ref(_cfg()), depth=None) == -1 and stats(ref(_cfg()), ident=None) == -1 and b"null" in lib.vmapstep_last_error()
    assert emit(None) == -1 and emit(ref(_cfg()), keys=None) == -1 and write(None) == -1 and write(ref(_cfg()), labels=None) == -1
    for bad in (dict(width=0), dict(n_background=-1), dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(n_det=33), dict(n_det=-1), dict(n_pairs=-1),
                dict(next_id=0), dict(next_id=65), dict(ratio_q=-1)):
        assert stats(ref(_cfg(**bad))) == -1 and emit(ref(_cfg(**bad))) == -1 and write(ref(_cfg(**bad))) == -1, bad
    for kw in limits:
        assert stats(ref(_cfg(**kw))) == -2 and emit(ref(_cfg(**kw))) == -2 and write(ref(_cfg(**kw))) == -2, kw
    assert stats(ref(_cfg()), ws=need - 1) == -3 and emit(ref(_cfg()), ws=need - 1) == -3 and b"track workspace" in lib.vmapstep_last_error()
    assert stats(ref(_cfg()), wsp=p + 64) == -3 and emit(ref(_cfg()), wsp=p + 64) == -3 and stats(ref(_cfg()), wsp=None) == -3       # misaligned, null
    assert stats(ref(_cfg(n_det=4096, n_pairs=65536, next_id=32767, **top)), ws=0) == -3      # at every limit: passes them
    assert lib.vmapstep_abi_version() == 7


def test_track_cfg_layout_matches_the_header(tmp_path):
    """The ctypes mirror of vmapstep_track_cfg against include/vmapstep.h as gcc lays it out; the constants and status values."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    from vmap_amd import tracking
    fields = [f for f, _ in _lib.TrackCfg._fields_]
    names = ["ABSENT", "NEW", "MERGED", "BACKGROUND", "FEW_POINTS", "SMALL", "NEW_NO_BOX"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmapstep.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(vmapstep_track_cfg));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(vmapstep_track_cfg, {f}));\n' for f in fields)
                   + '  printf("consts %d %d %d %d %d\\n", VMAPSTEP_TRACK_ROW_INTS, VMAPSTEP_TRACK_HEAD_INTS, VMAPSTEP_TRACK_MAX_DET, '
                     'VMAPSTEP_TRACK_MAX_PAIRS, VMAPSTEP_TRACK_PAIR_SLOTS);\n'
                   + '  printf("status' + " %d" * len(names) + '\\n", ' + ", ".join("VMAPSTEP_TRACK_" + s for s in names) + ");\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert int(got["size"][0]) == ctypes.sizeof(_lib.TrackCfg)
    for f in fields:
        assert int(got[f][0]) == getattr(_lib.TrackCfg, f).offset, f
    assert [int(x) for x in got["consts"]] == [_lib.TRACK_ROW_INTS, _lib.TRACK_HEAD_INTS, _lib.TRACK_MAX_DET, _lib.TRACK_MAX_PAIRS, _lib.TRACK_PAIR_SLOTS]
    assert to.ROW_INTS == _lib.TRACK_ROW_INTS
    assert [int(x) for x in got["status"]] == [getattr(tracking, s) for s in names] == [getattr(to, s) for s in names]


def test_instance_tracker_refuses_a_cpu_device_and_limits_out_of_range():
    from vmap_amd import tracking
    with pytest.raises(_lib.VmapStepError):
        tracking.InstanceTracker(75, 53, tc.INTRINSICS, 1e-3, 8.0, device="cpu")
    for kw in (dict(max_det=0), dict(max_det=4097), dict(max_pairs=65537), dict(max_ids=1), dict(max_ids=32768), dict(erode_radius=9),
               dict(voxel_size=0.0), dict(match_ratio=1.5), dict(background_classes=range(65))):
        with pytest.raises(ValueError):
            tracking.InstanceTracker(75, 53, tc.INTRINSICS, 1e-3, 8.0, **kw)
