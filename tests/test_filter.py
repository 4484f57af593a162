"""CPU tier of the instance filter: the numpy checker (tests/filter_oracle.py) against scipy's erosion and against itself on a
two-frame scenario, csrc/filter_rules.h - compiled into the host program tests/tools/filter_rules_host.cpp with the address and
undefined-behaviour sanitizers - against the checker bit for bit, and the argument checks of vmapstep_filter_* (no device is touched).
Neither Open3D nor OpenCV is involved anywhere: what is pinned is the contract of include/vmapstep.h."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import filter_cases as fc
import filter_oracle as fo
from conftest import ROOT
from vmap_amd import _lib


# ---- the erosion rule ---------------------------------------------------------------------------------------------------------------

def test_oracle_erosion_equals_three_iterations_of_a_5x5_erosion():
    """Radius 6 against scipy.ndimage.binary_erosion(mask, ones((5, 5)), iterations=3, border_value=1) - what three iterations of
    cv2.erode with a 5 x 5 kernel and the default border are taken to be - on random masks from 14 x 14 up, blobs on all four borders."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    cases = []
    for h, w in ((14, 14), (14, 31), (40, 17), (53, 75), (64, 64)):
        for fill in (0.999, 0.99, 0.9):
            cases.append(rng.random((h, w)) < fill)
        m = np.zeros((h, w), bool)                            # blobs that touch the top, bottom, left and right borders and a corner
        m[:h // 2, w // 4:] = True
        m[h // 3:, :w // 2] = True
        m[h // 2, w // 3] = False
        cases.append(m)
        cases.append(np.ones((h, w), bool))
    for m in cases:
        want = ndimage.binary_erosion(m, np.ones((5, 5)), iterations=3, border_value=1)
        assert np.array_equal(fo.erode(m, 6), want), m.shape
    assert any(fo.erode(m, 6).any() and not fo.erode(m, 6).all() for m in cases)
    m = cases[3]
    assert np.array_equal(fo.erode(m, 0), m) and np.array_equal(fo.erode(m, 2), ndimage.binary_erosion(m, np.ones((5, 5)), border_value=1))


def test_oracle_fused_multiply_add_is_exact():
    """fmaf against exact rational arithmetic, on operands chosen so that the float64 sum alone would round twice."""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-8, 3, 4000)).astype(np.float32)
    a[:3], b[:3], c[:3] = (1 + 2 ** -23, 3, 1e-3), (1 + 2 ** -23, 5, 7), (2.0 ** -60, -15, 1e-38)
    got = fo.fmaf(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo, hi = np.nextafter(np.float32(g), np.float32(-np.inf)), np.nextafter(np.float32(g), np.float32(np.inf))
        assert abs(Fraction(g) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), (x, y, z, g)


# ---- csrc/filter_rules.h on the host ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """A stand-alone program with its own main, built with -fsanitize=address,undefined: any out-of-bounds access or undefined
    arithmetic in the rules aborts it."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("filter_host") / "filter_rules_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vmap_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "filter_rules_host.cpp"), "-o", exe], check=True)
    return exe


def bits(x):
    return f"{int(np.float32(x).view(np.uint32)):08x}"


def run_host(exe, tmp_path, lines):
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(lines) + "\n")
    return subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]


def compare(exe, tmp_path, lines, want):
    got = run_host(exe, tmp_path, lines)
    asked = [l for l in lines if l[0] not in "BCT"]
    assert len(got) == len(want) == len(asked)
    bad = [(l, g, w) for l, g, w in zip(asked, got, want) if g != w]
    assert not bad, bad[:5]


def test_host_unprojection_and_depth_equal_the_oracle(host_exe, tmp_path):
    rng = np.random.default_rng(5)
    lines, want = [], []
    for k in range(40):                                       # cameras: a rotation from a QR, a translation of some metres
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = q, rng.standard_normal(3) * 3
        K = (float(rng.uniform(200, 700)), float(rng.uniform(200, 700)), float(rng.uniform(100, 400)), float(rng.uniform(100, 300)))
        lines.append("C " + " ".join(bits(x) for x in K) + " " + " ".join(bits(x) for x in T[:3].reshape(-1)))
        u, v = rng.integers(0, 640, 60), rng.integers(0, 480, 60)
        d = (rng.random(60) * 8).astype(np.float32)
        p = fo.world_points(u, v, d, K, T)
        for i in range(60):
            lines.append(f"P {u[i]} {v[i]} {bits(d[i])}")
            want.append(" ".join(bits(x) for x in p[i]))
    raws = np.concatenate([rng.integers(0, 65536, 300).astype(np.float32), (rng.random(300) * 12).astype(np.float32),
                           np.array([0.0, -1.0, 8.0, np.nextafter(np.float32(8.0), np.float32(9.0)), np.inf, -np.inf, np.nan], np.float32)])
    for i, raw in enumerate(raws):
        sc, mx = (np.float32(1.0 / 1000.0), np.float32(8.0)) if i < 300 else (np.float32(1.0), np.float32(8.0))
        d = fo.depth_of(np.array([raw]), sc, mx)[0]
        lines.append(f"D {bits(raw)} {bits(sc)} {bits(mx)}")
        with np.errstate(invalid="ignore"):
            want.append(f"{bits(d)} {int(d > 0)}")
    assert want[-1].endswith(" 0") and want[-7].split()[1] == "0" and want[-3] == f"{bits(0.0)} 0"      # NaN, depth 0 and beyond max_depth
    compare(host_exe, tmp_path, lines, want)


def test_host_voxel_keys_equal_the_oracle(host_exe, tmp_path):
    """Negative coordinates (floor, not truncation), both ends of the key range and one past, NaN and infinity; the key's fields and
    the centre a key stands for."""
    rng = np.random.default_rng(6)
    voxel = np.float32(0.01)
    pts = (rng.standard_normal((600, 3)) * 3).astype(np.float32)
    edge = np.float32(327.68)
    special = np.array([[-0.005, 0.005, -0.0], [-0.01, -0.010001, 0.01], [-327.68, 327.675, 0.0], [-327.69, 0.0, 0.0], [0.0, 327.68, 0.0],
                        [np.nextafter(-edge, np.float32(0)), np.nextafter(edge, np.float32(0)), 1.0], [0.0, 0.0, np.nan], [np.inf, 0.0, 0.0],
                        [0.0, -np.inf, 0.0], [1e30, 0.0, 0.0]], np.float32)
    pts = np.concatenate([pts, special])
    k, ok = fo.voxel_coords(pts, voxel)
    assert ok[600] and k[600].tolist() == [-1, 0, 0] and k[601].tolist() == [-1, -2, 1]                 # floor, not truncation
    assert ok[602] and k[602, 0] == -32768 and not ok[603] and not ok[604] and not ok[606:].any()
    lines, want, keys = [], [], []
    for i, (p, good) in enumerate(zip(pts, ok)):
        idv = int(rng.integers(0, 32767)) if i % 7 else 32766
        lines.append(f"K {idv} {bits(voxel)} " + " ".join(bits(x) for x in p))
        key = int(fo.pack_keys(idv, k[i]))
        want.append(f"1 {key}" if good else "0")
        if good:
            keys.append((key, idv, k[i]))
    for key, idv, kk in keys[:200] + keys[-5:]:
        lines.append(f"X {key}")
        want.append(f"{idv} {kk[0]} {kk[1]} {kk[2]}")
    for q in [-32768, -1, 0, 1, 32767] + rng.integers(-32768, 32768, 300).tolist():
        for vx in (voxel, np.float32(0.02), np.float32(0.037)):
            lines.append(f"V {q} {bits(vx)}")
            want.append(bits(fo.fmaf(np.float32(q), vx, np.float32(0.5) * vx)))
    assert np.array_equal(fo.key_points(np.array([keys[0][0]]), voxel)[0], fo.fmaf(keys[0][2].astype(np.float32), voxel, np.float32(0.5) * voxel))
    compare(host_exe, tmp_path, lines, want)


def test_host_inside_test_equals_the_oracle(host_exe, tmp_path):
    """Random boxes and points around their faces, and an axis-aligned box with points exactly on a face (inside), one float32 step
    beyond it (outside), and a NaN (outside)."""
    rng = np.random.default_rng(8)
    lines, want = [], []
    for _ in range(30):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        row = np.zeros(16, np.float32)
        row[0:3], row[3:12], row[12:15], row[15] = rng.standard_normal(3), q.T.reshape(9), rng.uniform(0.05, 1.0, 3), 1.0
        lines.append("T " + " ".join(bits(x) for x in row))
        local = rng.uniform(-1.2, 1.2, (80, 3)) * row[12:15]
        local[::4, 0] = row[12] * rng.choice([-1, 1], 20)     # near a face
        p = (row[0:3] + local @ q.T).astype(np.float32)
        inside = fo.inside_box(row, p)
        assert inside.any() and not inside.all()
        for i in range(80):
            lines.append("I " + " ".join(bits(x) for x in p[i]))
            want.append(str(int(inside[i])))
    row = np.zeros(16, np.float32)
    row[0:3], row[3:12], row[12:15], row[15] = (1.0, 2.0, 3.0), np.eye(3).reshape(9), (0.5, 0.25, 0.125), 1.0
    lines.append("T " + " ".join(bits(x) for x in row))
    beyond = np.nextafter(np.float32(1.5), np.float32(2))
    for p, w in (((1.5, 2.0, 3.0), 1), ((beyond, 2.0, 3.0), 0), ((0.5, 2.25, 3.125), 1), ((1.0, 2.0, np.float32(2.875)), 1),
                 ((1.0, np.nextafter(np.float32(1.75), np.float32(0)), 3.0), 0), ((np.nan, 2.0, 3.0), 0), ((1.0, 2.0, 3.0), 1)):
        assert int(fo.inside_box(row, np.array([p], np.float32))[0]) == w
        lines.append("I " + " ".join(bits(x) for x in p))
        want.append(str(w))
    compare(host_exe, tmp_path, lines, want)


def test_host_decisions_equal_the_oracle_on_every_branch(host_exe, tmp_path):
    rng = np.random.default_rng(9)
    bg = [1, 3, -1]
    lines, want = [f"B {len(bg)} " + " ".join(map(str, bg))], []
    for _ in range(3000):
        idv = int(rng.choice([0, 1, 2, 40, 32766]))
        min_pixels, min_points = int(rng.choice([30, 1500])), int(rng.choice([0, 10]))
        known = int(rng.random() < 0.5)
        pixels = 0 if rng.random() < 0.05 else int(rng.integers(1, 5000))
        c = int(rng.choice([-1, 1, 3, 7, 52]))
        c2 = c if rng.random() < 0.9 else c + int(rng.integers(1, 4))
        valid = int(rng.choice([0, 9, 10, 11, pixels]))
        inside = int(rng.choice([0, 1, valid])) if known else 0
        eroded = int(rng.choice([0, 29, 30, 31, 1499, 1500, pixels]))
        lines.append(f"R {idv} {min_pixels} {min_points} {known} {pixels} {c} {c2} {valid} {inside} {eroded}")
        want.append(str(fo.decide(idv, pixels, c, c2, valid, inside, eroded, bool(known), min_pixels, min_points, bg)))
    assert {int(w) for w in want} == {fo.ABSENT, fo.NEW, fo.MERGED, fo.UNSURE, fo.BACKGROUND, fo.FEW_POINTS, fo.SMALL, fo.MIXED}
    for idv in (1, 7, 63):
        for st in range(9):
            for valid in (0, 1):
                for inside in (0, 1):
                    lines.append(f"L {idv} {st} {valid} {inside}")
                    want.append(str(fo.label_of(idv, st, valid, inside)))
    for st in range(9):
        for flags in range(8):
            lines.append(f"E {st} {flags}")
            want.append(str(int((st == fo.NEW and flags & 5 == 5) or (st == fo.MERGED and flags & 3 == 3))))
    for raw, shift, n in ((0, 1, 64), (-1, 1, 64), (62, 1, 64), (63, 1, 64), (-2, 1, 64), (2147483647, 1, 64), (-2147483648, -1, 64), (65535, 0, 32767)):
        lines.append(f"S {raw} {shift} {n}")
        want.append(str(raw + shift if 0 <= raw + shift < n else -1))
    compare(host_exe, tmp_path, lines, want)


# ---- a two-frame scenario through the checker, the boxes from the numpy backend of the search ---------------------------------------

def oracle_filter(radius=6):
    s = fc.SETTINGS
    return fo.Filter(fc.W, fc.H, fc.INTRINSICS, s["depth_scale"], s["max_depth"], s["background"], s["min_pixels"], s["min_points"], radius,
                     s["voxel_size"], 0, s["max_ids"])


def register(table, flt, out, margin):
    """What InstanceFilter does after a frame, with the numpy backend of the box search."""
    from vmap_amd import bounds, instances
    for i, st in zip(out["rows"][:, 0].tolist(), out["rows"][:, 1].tolist()):
        if st in (fo.NEW, fo.MERGED):
            keys = flt.keys[(flt.keys >> 48) == i]
            box = bounds.oriented_bounds(fo.key_points(keys, flt.voxel), backend="numpy", min_extent=0.0)[0]
            assert box is not None
            table[i] = instances.box_row(box, margin)


def test_two_frames_through_the_oracle_produce_every_status():
    frames = fc.sequence()
    flt = oracle_filter()
    table = np.zeros((fc.MAX_IDS, 16), np.float32)
    ids, sem, depth, t_wc = frames[0]
    one = flt.put(depth, ids, sem, t_wc, table)
    st = dict(zip(one["rows"][:, 0].tolist(), one["rows"][:, 1].tolist()))
    assert st == {0: fo.BACKGROUND, fc.ID_NEW: fo.NEW, fc.ID_CORNER: fo.NEW, fc.ID_STRIP: fo.SMALL, fc.ID_FILL: fo.BACKGROUND, fc.ID_LEFT: fo.NEW,
                  fc.ID_RIGHT: fo.NEW, fc.ID_FEW: fo.FEW_POINTS, fc.ID_RIM: fo.NEW_NO_BOX, fc.ID_LAST: fo.SMALL}
    rows = {int(r[0]): r for r in one["rows"]}
    assert rows[fc.ID_NEW][6] == 11 * 11 - 9 and rows[fc.ID_CORNER][6] == 100 and rows[fc.ID_STRIP][6] == 0      # the hole; the corner; the strip
    assert rows[fc.ID_RIM][6] == 11 * 17 and rows[fc.ID_RIM][7] == 0 and rows[fc.ID_FEW][4] == 10
    assert rows[fc.ID_LEFT][6] == rows[fc.ID_RIGHT][6] == 8 * 11
    assert one["overflow"] == 0 and one["out_of_grid"] == 0 and not one["mixed"]
    assert set(np.unique(one["labels"]).tolist()) == {0, fc.ID_NEW, fc.ID_CORNER, fc.ID_LEFT, fc.ID_RIGHT}
    assert set((flt.keys >> 48).tolist()) == {fc.ID_NEW, fc.ID_CORNER, fc.ID_LEFT, fc.ID_RIGHT}
    register(table, flt, one, 0.875 * flt.voxel)
    ids, sem, depth, t_wc = frames[1]
    two = flt.put(depth, ids, sem, t_wc, table)
    st2 = dict(zip(two["rows"][:, 0].tolist(), two["rows"][:, 1].tolist()))
    assert st2[fc.ID_NEW] == fo.MERGED and st2[fc.ID_CORNER] == fo.UNSURE and st2[fc.ID_LATE] == fo.NEW and st2[fc.ID_RIM] == fo.NEW_NO_BOX
    assert set(st.values()) | set(st2.values()) == {fo.NEW, fo.MERGED, fo.UNSURE, fo.BACKGROUND, fo.FEW_POINTS, fo.SMALL, fo.NEW_NO_BOX}
    lab = two["labels"][ids == fc.ID_NEW]
    assert (lab == fc.ID_NEW).any() and (lab == -1).any() and set(lab.tolist()) == {fc.ID_NEW, -1}
    assert (two["labels"][ids == fc.ID_CORNER] == -1).all()
    assert two["labels"][10, 45] == fc.ID_NEW                 # a pixel of a MERGED mask with depth 0 keeps the id
    # radius 2: the strip survives, the rim's eroded region reaches valid pixels
    small = oracle_filter(2).put(frames[0][2], frames[0][0], frames[0][1], frames[0][3], np.zeros((fc.MAX_IDS, 16), np.float32))
    st = dict(zip(small["rows"][:, 0].tolist(), small["rows"][:, 1].tolist()))
    assert st[fc.ID_STRIP] == fo.NEW and st[fc.ID_RIM] == fo.NEW and st[fc.ID_LAST] == fo.NEW
    # a mixed class, an id out of range and a point beyond the key range
    sem_bad = frames[0][1].copy()
    sem_bad[3, 3] += 1
    bad = oracle_filter().put(frames[0][2], frames[0][0], sem_bad, frames[0][3], table)
    assert bad["mixed"] == [fc.ID_CORNER]
    ids_bad = frames[0][0].copy()
    ids_bad[0, 0] = fc.MAX_IDS
    assert oracle_filter().put(frames[0][2], ids_bad, frames[0][1], frames[0][3], table)["overflow"] == 1
    far = oracle_filter().put(frames[0][2], frames[0][0], frames[0][1], fc.pose(tx=700.0), np.zeros((fc.MAX_IDS, 16), np.float32))
    assert far["out_of_grid"] > 0 and len(far["frame_keys"]) == 0


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

def _cfg(width=75, height=53, max_ids=64, erode_radius=6, n_background=2, voxel_size=0.01):
    bg = (ctypes.c_int32 * 64)(1, 3)
    pose = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
    return _lib.FilterCfg(width, height, 0, 0, 1.0 / 1000.0, 8.0, 60.0, 60.0, 37.0, 26.0, pose, voxel_size, 1, 30, 10, erode_radius, max_ids,
                          n_background, bg)


def test_abi_refuses_bad_arguments_before_anything_is_enqueued():
    """One call per return code, none of which reads a pointer or touches a device: -1 for null or inconsistent arguments, -2 past a
    limit, -3 for a short workspace - which is also as far as a well-formed call gets here."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    n = ctypes.c_size_t()
    ref = ctypes.byref
    assert lib.vmapstep_filter_workspace_bytes(ref(_cfg()), ref(n)) == 0 and n.value >= 8 * 64 * 8 * 4 + 75 * 53
    need = n.value
    assert lib.vmapstep_filter_workspace_bytes(ref(_cfg(max_ids=32767, width=4095, height=4095, erode_radius=8)), ref(n)) == 0 and n.value > need
    assert lib.vmapstep_filter_workspace_bytes(ref(_cfg()), None) == -1 and lib.vmapstep_filter_workspace_bytes(None, ref(n)) == -1
    limits = (dict(max_ids=1), dict(max_ids=32768), dict(erode_radius=-1), dict(erode_radius=9), dict(width=4096), dict(height=4096), dict(n_background=65))
    for kw in limits:
        assert lib.vmapstep_filter_workspace_bytes(ref(_cfg(**kw)), ref(n)) == -2 and b"filter limits" in lib.vmapstep_last_error(), kw
    stats = lambda cfg, ws=need, depth=p, status=p: lib.vmapstep_filter_stats(cfg, depth, p, p, p, status, p, p, ws, None)
    emit = lambda cfg, ws=need, keys=p: lib.vmapstep_filter_emit(cfg, p, p, p, keys, p, p, ws, None)
    write = lambda cfg, labels=p: lib.vmapstep_filter_write(cfg, p, p, p, p, labels, None)
    assert stats(None) == -1 and stats(ref(_cfg()), depth=None) == -1 and stats(ref(_cfg()), status=None) == -1 and b"null" in lib.vmapstep_last_error()
    assert emit(None) == -1 and emit(ref(_cfg()), keys=None) == -1 and write(None) == -1 and write(ref(_cfg()), labels=None) == -1
    for bad in (dict(width=0), dict(n_background=-1), dict(voxel_size=0.0), dict(voxel_size=float("nan"))):
        assert stats(ref(_cfg(**bad))) == -1 and emit(ref(_cfg(**bad))) == -1 and write(ref(_cfg(**bad))) == -1, bad
    for kw in limits:
        assert stats(ref(_cfg(**kw))) == -2 and emit(ref(_cfg(**kw))) == -2 and write(ref(_cfg(**kw))) == -2, kw
    assert stats(ref(_cfg()), ws=need - 1) == -3 and emit(ref(_cfg()), ws=need - 1) == -3 and b"filter workspace" in lib.vmapstep_last_error()
    assert stats(ref(_cfg(max_ids=32767, width=4095, height=4095, erode_radius=8)), ws=0) == -3      # at every limit: passes them
    assert lib.vmapstep_voxel_points(None, 0, p, 1, 0.01, p, p, None) == -1 and lib.vmapstep_voxel_points(p, 0, p, 0, 0.01, p, p, None) == -1
    assert lib.vmapstep_voxel_points(p, -1, p, 1, 0.01, p, p, None) == -1 and lib.vmapstep_voxel_points(p, 0, p, 1, 0.0, p, p, None) == -1
    assert lib.vmapstep_abi_version() == 7


def test_filter_cfg_layout_matches_the_header(tmp_path):
    """The ctypes mirror of vmapstep_filter_cfg against include/vmapstep.h as gcc lays it out; the status values against the module's."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    from vmap_amd import instances
    fields = [f for f, _ in _lib.FilterCfg._fields_]
    names = ["ABSENT", "NEW", "MERGED", "UNSURE", "BACKGROUND", "FEW_POINTS", "SMALL", "MIXED", "NEW_NO_BOX"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmapstep.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(vmapstep_filter_cfg));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(vmapstep_filter_cfg, {f}));\n' for f in fields)
                   + '  printf("consts %d %d %d %d\\n", VMAPSTEP_FILTER_MAX_CLASSES, VMAPSTEP_FILTER_ROW_INTS, VMAPSTEP_FILTER_HEAD_INTS, VMAPSTEP_FILTER_BOX_FLOATS);\n'
                   + '  printf("status' + " %d" * 9 + '\\n", ' + ", ".join("VMAPSTEP_FILTER_" + s for s in names) + ");\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert int(got["size"][0]) == ctypes.sizeof(_lib.FilterCfg)
    for f in fields:
        assert int(got[f][0]) == getattr(_lib.FilterCfg, f).offset, f
    assert [int(x) for x in got["consts"]] == [_lib.FILTER_MAX_CLASSES, _lib.FILTER_ROW_INTS, _lib.FILTER_HEAD_INTS, _lib.FILTER_BOX_FLOATS]
    assert [int(x) for x in got["status"]] == list(range(9)) == [getattr(instances, s) for s in names] == [getattr(fo, s) for s in names]
    assert instances.STATUS_NAMES == tuple(names)


def test_instance_filter_refuses_a_cpu_device_and_bad_limits():
    from vmap_amd import instances
    with pytest.raises(_lib.VmapStepError):
        instances.InstanceFilter(75, 53, fc.INTRINSICS, 1e-3, 8.0, device="cpu")


def test_oriented_bounds_min_extent_keyword():
    """The new keyword: the default is the present floor, 0.0 leaves the found extents."""
    from vmap_amd import bounds
    rng = np.random.default_rng(2)
    pts = (rng.random((200, 3)) * np.array([0.5, 0.03, 0.2])).astype(np.float32)
    a = bounds.oriented_bounds(pts, backend="numpy")[0]
    b = bounds.oriented_bounds(pts, backend="numpy", min_extent=0.0)[0]
    assert a.extent.min() == bounds.MIN_EXTENT and 0 < b.extent.min() < 0.04
    assert np.array_equal(a.R, b.R) and np.array_equal(a.center, b.center) and np.array_equal(a.extent, np.maximum(b.extent, bounds.MIN_EXTENT))
