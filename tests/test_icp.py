"""CPU tier of the depth tracker: csrc/icp_rules.h - compiled into the stand-alone host program tests/tools/icp_rules_host.cpp with the
address and undefined-behaviour sanitizers - against the exact layer of the numpy checker (tests/icp_oracle.py) bit for bit on every
branch of the contract; the exact layer against the plain float64 Gauss-Newton layer and the true pose of the analytic scene; and the
argument checks of the icp entries of the C ABI (no device is touched).  Nothing is held against an outside implementation: the
contract of include/vmapstep.h is this project's own."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_cases as ic
import icp_oracle as io
from conftest import ROOT
from vmap_amd import _lib

f32 = np.float32
P = ic.PARAMS


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """A stand-alone program with its own main, built with -fsanitize=address,undefined."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("icp_host") / "icp_rules_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vmap_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "icp_rules_host.cpp"), "-o", exe], check=True)
    return exe


def h32(a):
    return " ".join(f"{x:08x}" for x in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32).tolist())


def h64(a):
    return " ".join(f"{x:016x}" for x in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64).tolist())


def from64(tokens):
    return np.array([int(t, 16) for t in tokens], np.uint64).view(np.float64)


def from32(tokens):
    return np.array([int(t, 16) for t in tokens], np.uint32).view(f32)


def run(exe, tmp_path, lines):
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(lines) + "\n")
    return subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.split("\n")


def head(p, intrinsics, width, height):
    return [f"R {h32([p.min_depth, p.max_depth, p.band, p.dist_thresh, p.cos_thresh])}", f"C {h32(intrinsics)} {width} {height}"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else a.view(np.uint64) if a.dtype == np.float64 else a


def dirty(depth, seed):
    """The scene's depth with a NaN, an inf, a -inf, zeros, a negative value and a block past max_depth."""
    d = depth.copy()
    rng = np.random.default_rng(seed)
    W, H = d.shape
    for v in (np.nan, np.inf, -np.inf, 0.0, 0.0, -1.0, 0.05, 11.0):
        d[rng.integers(W), rng.integers(H)] = v
    d[W // 2:W // 2 + 3, H // 3:H // 3 + 2] = 0.0
    return d


@pytest.mark.parametrize("width,height,levels", [(64, 48, 3), (37, 29, 3), (8, 8, 1), (5, 3, 2)])
def test_host_maps_equal_the_exact_checker(host_exe, tmp_path, width, height, levels):
    """Pyramid, level cameras and normal maps: odd sizes with clamped blocks, NaN / inf / 0 depths, the sphere's silhouette as a depth
    edge inside 2 x 2 blocks and across central differences."""
    sc = ic.corner_scene(width, height)
    depth = dirty(sc["depth"], width)
    want = io.maps(depth, sc["intrinsics"], levels, P)
    lines = head(P, sc["intrinsics"], width, height) + [f"K {l}" for l in range(levels)] + [f"M {levels} {h32(depth)}"]
    out = run(host_exe, tmp_path, lines)
    for l in range(levels):
        tok = out[l].split()
        assert np.array_equal(from32(tok[:4]).view(np.uint32), bits(np.array(io.level_camera(sc["intrinsics"], l), f32)))
        assert (int(tok[4]), int(tok[5])) == want[l].shape[:2]
    at = levels
    for l in range(levels):
        W, H = want[l].shape[:2]
        assert out[at].split() == ["level", str(l), str(W), str(H)]
        got = from32(" ".join(out[at + 1:at + 1 + W * H]).split()).reshape(W, H, 4)
        assert np.array_equal(bits(got), bits(want[l])), l
        at += 1 + W * H
    if width >= 37:
        normals = [(m[..., :3] != 0).any(-1) for m in want]
        assert all(n.mean() > 0.3 for n in normals)
        assert not normals[0][[0, -1]].any() and not normals[0][:, [0, -1]].any()         # border pixels have no normal
        assert ((want[0][..., 3] > 0) & ~normals[0])[1:-1, 1:-1].any()                     # a valid depth without a normal: an edge
        for l, m in enumerate(want):                                                      # towards the camera
            v = io.vertex(io.level_camera(sc["intrinsics"], l), *np.meshgrid(np.arange(m.shape[0]), np.arange(m.shape[1]), indexing="ij"), m[..., 3])
            assert ((m[..., 0] * v[0] + m[..., 1] * v[1] + m[..., 2] * v[2]) <= 0).all()


def test_a_depth_edge_is_never_averaged():
    """Section 1 by hand: a 2 x 2 block with max - min > band gives 0; within the band the mean of the valid ones in order."""
    D = np.array([[1.0, 1.2], [1.1, 0.0]], f32)
    assert io.down(D, P)[0, 0] == (f32(1.0) + f32(1.1) + f32(1.2)) / f32(3)
    D[1, 1] = 1.3
    assert io.down(D, P)[0, 0] == 0.0
    assert io.down(np.zeros((3, 3), f32), P).shape == (2, 2)
    edge = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.6]], f32)
    assert io.down(edge, P)[1, 1] == f32(1.6)                                              # a clamped corner: the pixel four times


def frame_lines(level, T, src, model):
    return [f"F {level} {h64(T)}", h32(src), h32(model)]


def parse_frame(out, W, H):
    rows = [l.split() for l in out[:W * H]]
    reason = np.array([int(r[0]) for r in rows]).reshape(W, H)
    r = from64([r[1] for r in rows]).reshape(W, H)
    J = from64([t for r in rows for t in r[2:8]]).reshape(W, H, 6)
    tail = out[W * H].split()
    assert tail[0] == "sums"
    return reason, r, J, np.array([int(t) for t in tail[1:]], np.int64)


@pytest.mark.parametrize("width,height", [(64, 48), (37, 29)])
def test_host_correspondences_and_sums_equal_the_exact_checker(host_exe, tmp_path, width, height):
    """Every level of the corner scene under the initial and the true pose: reason, r, J per pixel and the 29 integers."""
    sc = ic.corner_scene(width, height)
    src, mod = io.maps(dirty(sc["depth"], 1), sc["intrinsics"], 3, P), io.maps(sc["model_depth"], sc["intrinsics"], 3, P)
    seen = set()
    for level in range(3):
        for T in (sc["T_init"], sc["T_true"]):
            cam = io.level_camera(sc["intrinsics"], level)
            reason, r, J = io.correspond(src[level], mod[level], cam, T, P)
            W, H = reason.shape
            got = parse_frame(run(host_exe, tmp_path, head(P, sc["intrinsics"], width, height) + frame_lines(level, T, src[level], mod[level])), W, H)
            assert np.array_equal(got[0], reason)
            live = reason == io.INLIER
            assert np.array_equal(bits(got[1][live]), bits(r[live])) and np.array_equal(bits(got[2][live]), bits(J[live]))
            assert np.array_equal(got[3], io.sums(src[level], mod[level], cam, T, P))
            assert got[3][0] == live.sum() > 20
            seen |= set(np.unique(reason).tolist())
    assert {io.INLIER, io.NO_NORMAL, io.NO_MODEL, io.ANGLE} <= seen                      # FAR, OUTSIDE, GUARD: the lone-pixel cases below


def one_pixel(src_entry, model_entry, W=5, H=5, at=(2, 2)):
    src, model = np.zeros((W, H, 4), f32), np.zeros((W, H, 4), f32)
    src[at] = src_entry
    model[...] = model_entry
    return src, model


LONE = dict(min_depth=0.1, max_depth=1000.0, band=0.25, dist_thresh=0.125, cos_thresh=0.75)
LONE_CASES = [  # name, source entry, model entry, translation, the reason
    ("inlier", (0, 0, -1, 2.0), (0, 0, -1, 2.0), (0, 0, 0.05), io.INLIER),
    ("no_normal", (0, 0, 0, 2.0), (0, 0, -1, 2.0), (0, 0, 0), io.NO_NORMAL),
    ("behind", (0, 0, -1, 2.0), (0, 0, -1, 2.0), (0, 0, -1.95), io.OUTSIDE),
    ("out_of_image", (0, 0, -1, 2.0), (0, 0, -1, 2.0), (3.0, 0, 0), io.OUTSIDE),
    ("no_model", (0, 0, -1, 2.0), (0, 0, 0, 2.0), (0, 0, 0), io.NO_MODEL),
    ("far", (0, 0, -1, 2.0), (0, 0, -1, 2.2), (0, 0, 0), io.FAR),
    ("at_dist_thresh", (0, 0, -1, 2.0), (0, 0, -1, 2.125), (0, 0, 0), io.INLIER),
    ("angle", (0, 0, -1, 2.0), (0.8, 0, -0.6, 2.0), (0, 0, 0), io.ANGLE),
    ("at_cos_thresh", (0, 0, -1, 2.0), (0.6614, 0, -0.75, 2.0), (0, 0, 0), io.INLIER),
    ("at_guard", (1, 0, 0, 64.0), (1, 0, 0, 64.0), (0, 0, 0), io.INLIER),              # J4 = z * m0 = 64 exactly: admitted
    ("past_guard", (1, 0, 0, 64.0), (1, 0, 0, float(np.nextafter(f32(64), f32(65)))), (0, 0, float(np.nextafter(f32(64), f32(65))) - 64.0), io.GUARD),
]


@pytest.mark.parametrize("name,src_entry,model_entry,trans,want", LONE_CASES, ids=[c[0] for c in LONE_CASES])
def test_each_rejection_reason_alone(host_exe, tmp_path, name, src_entry, model_entry, trans, want):
    """One source pixel at the principal point against a constant model map: each reason by itself, and the thresholds and the guard of
    64 met exactly (<=, >=: admitted) and passed by one unit in the last place."""
    p = io.Params(**LONE)
    intr = (10.0, 10.0, 2.0, 2.0)
    src, model = one_pixel(src_entry, model_entry)
    T = np.eye(4)[:3].copy()
    T[:, 3] = trans
    cam = io.level_camera(intr, 0)
    reason, r, J = io.correspond(src, model, cam, T.reshape(12), p)
    assert reason[2, 2] == want and (np.delete(reason.reshape(-1), 12) == io.NO_NORMAL).all()
    got = parse_frame(run(host_exe, tmp_path, head(p, intr, 5, 5) + frame_lines(0, T, src, model)), 5, 5)
    assert np.array_equal(got[0], reason)
    assert np.array_equal(got[3], io.sums(src, model, cam, T.reshape(12), p)) and got[3][0] == (want == io.INLIER)
    if want in (io.INLIER, io.GUARD):
        assert np.array_equal(bits(got[1][2, 2:3]), bits(r[2, 2:3])) and np.array_equal(bits(got[2][2, 2]), bits(J[2, 2]))
    if name == "at_guard":
        assert J[2, 2, 4] == 64.0 and got[3][1 + 15 + 3] == 2 ** 42                  # (4, 4) of J J^T: 64 * 64 * 2^30
    if name == "past_guard":
        assert abs(J[2, 2, 4]) > 64.0


def solve_line(p, s, T):
    return f"S {h64([p.damping, p.pivot_rel, p.eps])} {int(p.min_inliers)} {' '.join(str(int(v)) for v in s)} {h64(T)}"


def parse_solve(line):
    tok = line.split()
    return int(tok[0]), int(tok[1]), from64(tok[2:3])[0], from64(tok[3:9]), from64(tok[9:21])


def same_solve(got, want):
    status, finished, x, x2, T = want
    assert (got[0], got[1]) == (status, finished)
    assert np.array_equal(bits(np.float64(got[2]).reshape(1)), bits(np.float64(x2).reshape(1)))
    assert np.array_equal(bits(got[3]), bits(np.array(x, np.float64))) and np.array_equal(bits(got[4]), bits(np.array(T, np.float64)))


def diag_sums(diag, b=(0,) * 6, count=100):
    """The 29 integers of A = diag(diag), b, in units of 2^-30."""
    s = np.zeros(29, np.int64)
    s[0] = count
    at = 1
    for i in range(6):
        for j in range(i, 6):
            if i == j:
                s[at] = diag[i]
            at += 1
    s[22:28] = b
    return s


def test_host_solve_equals_the_exact_checker_on_every_branch(host_exe, tmp_path):
    """LDL^T and the Cayley update on the scene's own sums (all three levels, a damped one too), then the branches: count at and one
    below min_inliers, a pivot exactly at the threshold and one unit above it, the eps flag at and below |x|^2 = eps^2, a single plane."""
    sc = ic.corner_scene(64, 48)
    src, mod = io.maps(sc["depth"], sc["intrinsics"], 3, P), io.maps(sc["model_depth"], sc["intrinsics"], 3, P)
    cases = []
    for level in range(3):
        s = io.sums(src[level], mod[level], io.level_camera(sc["intrinsics"], level), sc["T_init"], P)
        cases.append((P, s, sc["T_init"]))
        cases.append((io.Params(damping=0.5), s, sc["T_true"]))
    n = int(cases[0][1][0])
    at_count = (io.Params(min_inliers=n), cases[0][1], sc["T_init"])
    below_count = (io.Params(min_inliers=n + 1), cases[0][1], sc["T_init"])
    q = 2 ** 30
    quarter = io.Params(pivot_rel=0.25, min_inliers=1)
    at_pivot = (quarter, diag_sums([4 * q, q, 2 * q, 2 * q, 2 * q, 2 * q], b=[q // 8] * 6), sc["T_true"])
    past_pivot = (quarter, diag_sums([4 * q, q + 1, 2 * q, 2 * q, 2 * q, 2 * q], b=[q // 8] * 6), sc["T_true"])
    tiny = diag_sums([q] * 6, b=[-(q >> 10), 0, 0, 0, 0, 0])                             # x = (2^-10, 0 ..): |x|^2 = 2^-20
    at_eps = (io.Params(eps=2.0 ** -10, min_inliers=1), tiny, sc["T_init"])
    below_eps = (io.Params(eps=float(np.nextafter(2.0 ** -10, 1.0)), min_inliers=1), tiny, sc["T_init"])
    plane_src, plane_mod = (io.maps(ic.corner_scene(64, 48, sphere=False, planes=(2,))[k], sc["intrinsics"], 1, P) for k in ("depth", "model_depth"))
    plane = (P, io.sums(plane_src[0], plane_mod[0], io.level_camera(sc["intrinsics"], 0), sc["T_init"], P), sc["T_init"])
    cases += [at_count, below_count, at_pivot, past_pivot, at_eps, below_eps, plane]
    out = run(host_exe, tmp_path, [solve_line(*c) for c in cases])
    want = [io.solve(s, T, p) for p, s, T in cases]
    for line, w in zip(out, want):
        same_solve(parse_solve(line), w)
    assert [w[0] for w in want[:6]] == [io.OK] * 6
    assert want[6][0] == io.OK and want[7][0] == io.DEGENERATE                            # count == min_inliers, min_inliers - 1
    assert want[8][0] == io.DEGENERATE and want[9][0] == io.OK                            # the pivot at the threshold, one unit above
    assert np.array_equal(np.array(want[8][4]), sc["T_true"])                             # DEGENERATE: the pose does not move
    assert (want[10][0], want[10][1], want[10][3]) == (io.OK, 0, 2.0 ** -20)              # |x|^2 == eps^2: not finished (<)
    assert (want[11][0], want[11][1]) == (io.OK, 1)
    assert plane[1][0] > 500 and want[12][0] == io.DEGENERATE and np.isfinite(want[12][4]).all()   # rank-deficient: the pivot test


def test_cayley_rotation_is_orthonormal(host_exe, tmp_path):
    """R of the Cayley map for |omega| up to 0.5, through the host program's solve (A = I, b = -omega, T = I): bit-equal to the
    checker's and orthonormal to 1e-15."""
    rng = np.random.default_rng(5)
    q = 2 ** 30
    p = io.Params(min_inliers=1)
    omegas = [rng.normal(size=3) for _ in range(40)]
    omegas = [w / np.linalg.norm(w) * s for w, s in zip(omegas, np.linspace(0.0, 0.5, 40))]
    cases = [(p, diag_sums([q] * 6, b=[0, 0, 0] + [-int(v) for v in np.rint(w * q)]), np.eye(4)[:3].reshape(12)) for w in omegas]
    out = run(host_exe, tmp_path, [solve_line(*c) for c in cases])
    for line, (pp, s, T), w in zip(out, cases, omegas):
        got = parse_solve(line)
        same_solve(got, io.solve(s, T, pp))
        R = got[4].reshape(3, 4)[:, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-15
        assert np.abs(got[3][3:] - np.rint(w * q) / q).max() == 0                      # A = I: x is -b exactly
        assert np.abs(R - io.rodrigues(2 * np.arctan(np.linalg.norm(got[3][3:]) / 2) * w / max(np.linalg.norm(w), 1e-300))).max() < 1e-9


def test_the_sums_reach_two_to_the_62_and_do_not_pass_it(host_exe, tmp_path):
    """The worst admissible input: 2^20 pixels with a product of 64 * 64.  The sum is 2^62 exactly, in both signs; the undefined-
    behaviour sanitizer would abort the program on a signed overflow."""
    out = run(host_exe, tmp_path, [f"Q {h64([4096.0])} {1 << 20}", f"Q {h64([-4096.0])} {1 << 20}", f"Q {h64([0.5 * 2.0 ** -30])} 3",
                                   f"Q {h64([1.5 * 2.0 ** -30])} 3"])
    assert [int(v) for v in out[:4]] == [2 ** 62, -2 ** 62, 0, 6]                        # half to even: 0.5 -> 0, 1.5 -> 2
    assert io.quant(64.0 * 64.0) * io.MAX_PIXELS == 2 ** 62 and io.MAX_PIXELS == _lib.ICP_MAX_PIXELS


def test_convergence_of_the_checker_on_the_corner_scene():
    """From 2 cm and 1 degree at 64 x 48: the plain float64 layer cuts the error at least tenfold; the exact layer - float32 maps, sums
    quantised to 2^-30 - stays within twice the recorded ratio of it; the recorded figures are the measured ones."""
    sc = ic.corner_scene(64, 48)
    exact = io.track(sc["depth"], sc["model_depth"], sc["T_init"], sc["intrinsics"], ic.ITERATIONS, P)
    plain = io.track_plain(sc["depth"], sc["model_depth"], sc["T_init"], sc["intrinsics"], ic.ITERATIONS, P)
    e0, e_plain, e_exact = io.pose_error(sc["T_init"], sc["T_true"]), io.pose_error(plain, sc["T_true"]), io.pose_error(exact["pose"], sc["T_true"])
    print(f"initial {e0:.6e} plain {e_plain:.6e} exact {e_exact:.6e} ratio {e_exact / e_plain:.6f}")
    assert e_plain * 10 <= e0
    assert e_exact <= 2 * ic.EXACT_OVER_PLAIN * e_plain
    for got, rec in ((e0, ic.INITIAL_ERROR), (e_plain, ic.PLAIN_ERROR), (e_exact, ic.EXACT_ERROR), (e_exact / e_plain, ic.EXACT_OVER_PLAIN)):
        assert abs(got - rec) <= 0.01 * rec
    assert io.summary(exact, ic.ITERATIONS[0], 64 * 48)[0]
    assert (exact["log"][:, 2] == io.SKIPPED).any() and not (exact["log"][:, 2] == io.DEGENERATE).any()


def cfg(**kw):
    base = dict(width=64, height=48, levels=3, min_inliers=12, iterations=(ctypes.c_int32 * 4)(4, 5, 10, 0), grid_cap=0, fx=60.0, fy=60.0, cx=31.5,
                cy=23.5, min_depth=0.1, max_depth=10.0, band=0.25, dist_thresh=0.15, cos_thresh=0.8, damping=0.0, pivot_rel=1e-6, eps=1e-6)
    base.update(kw)
    return _lib.IcpCfg(**base)


def test_struct_layout_matches_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmapstep.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(vmapstep_icp_cfg), offsetof(vmapstep_icp_cfg, iterations), offsetof(vmapstep_icp_cfg, fx),\n'
                   '         offsetof(vmapstep_icp_cfg, cos_thresh), offsetof(vmapstep_icp_cfg, damping));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C = _lib.IcpCfg
    assert got == [ctypes.sizeof(C), C.iterations.offset, C.fx.offset, C.cos_thresh.offset, C.damping.offset]


def test_icp_entries_check_their_arguments_without_a_device():
    """Refused before anything is enqueued; no pointer is read (the buffers here are host memory)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(2048)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    n = ctypes.c_size_t()
    assert lib.vmapstep_icp_maps_bytes(ctypes.byref(cfg()), ctypes.byref(n)) == 0 and n.value == 16 * (64 * 48 + 32 * 24 + 16 * 12)
    assert lib.vmapstep_icp_maps_bytes(ctypes.byref(cfg(width=37, height=29)), ctypes.byref(n)) == 0 and n.value == 16 * (37 * 29 + 19 * 15 + 10 * 8)
    assert lib.vmapstep_icp_maps_bytes(ctypes.byref(cfg(width=1024, height=1024)), ctypes.byref(n)) == 0                     # 2^20: the bound itself
    assert lib.vmapstep_icp_maps_bytes(ctypes.byref(cfg(width=1025, height=1024)), ctypes.byref(n)) == -2 and b"overflow" in lib.vmapstep_last_error()
    assert lib.vmapstep_icp_maps_bytes(None, ctypes.byref(n)) == -1 and lib.vmapstep_icp_maps_bytes(ctypes.byref(cfg()), None) == -1
    bad = [dict(levels=0), dict(levels=5), dict(width=0), dict(fx=0.0), dict(cx=float("nan")), dict(min_depth=-1.0), dict(max_depth=float("inf")),
           dict(max_depth=0.05), dict(band=-1.0), dict(dist_thresh=float("nan")), dict(damping=-1.0), dict(pivot_rel=float("nan")), dict(eps=-1.0),
           dict(min_inliers=-1), dict(grid_cap=-1)]
    for kw in bad:
        assert lib.vmapstep_icp_pyramid(ctypes.byref(cfg(**kw)), p, p, None) == -1, kw
        assert lib.vmapstep_icp_track(ctypes.byref(cfg(**kw)), p, p, p, p, p, p, p, None) == -1, kw
    assert lib.vmapstep_icp_pyramid(ctypes.byref(cfg()), None, p, None) == -1 and lib.vmapstep_icp_pyramid(ctypes.byref(cfg()), p, None, None) == -1
    assert lib.vmapstep_icp_pyramid(ctypes.byref(cfg()), p, p + 8, None) == -3
    assert lib.vmapstep_icp_sums(ctypes.byref(cfg()), p, p, 3, p, p, None) == -1 and b"level=3" in lib.vmapstep_last_error()
    assert lib.vmapstep_icp_sums(ctypes.byref(cfg()), p, p, -1, p, p, None) == -1
    assert lib.vmapstep_icp_sums(ctypes.byref(cfg()), p, p, 0, p + 4, p, None) == -1
    assert lib.vmapstep_icp_sums(ctypes.byref(cfg()), p + 4, p, 0, p, p, None) == -3
    for its in ((0, 5, 10, 0), (4, 65, 10, 0), (4, 5, -1, 0)):
        assert lib.vmapstep_icp_track(ctypes.byref(cfg(iterations=(ctypes.c_int32 * 4)(*its))), p, p, p, p, p, p, p, None) == -1
        assert b"iterations" in lib.vmapstep_last_error()
    assert lib.vmapstep_icp_pyramid(ctypes.byref(cfg(iterations=(ctypes.c_int32 * 4)(0, 0, 0, 0))), p, p + 8, None) == -3   # not the pyramid's business
    assert lib.vmapstep_icp_track(ctypes.byref(cfg()), p, p, None, p, p, p, p, None) == -1
    assert lib.vmapstep_icp_track(ctypes.byref(cfg()), p, p, p, p, p, p, p + 128, None) == -3 and b"state" in lib.vmapstep_last_error()
    assert lib.vmapstep_icp_track(ctypes.byref(cfg(width=2048, height=1024)), p, p, p, p, p, p, p, None) == -2
    assert _lib.ICP_STATE_BYTES == 512 and _lib.ICP_SUMS == 29


def test_odometry_refuses_bad_arguments_without_a_device():
    import torch
    from vmap_amd import odometry
    assert odometry.level_sizes(37, 29, 3) == [(37, 29), (19, 15), (10, 8)]
    with pytest.raises(TypeError):
        odometry.DepthTracker((10, 10, 4, 4), 8, 8, (2,), no_such_argument=1)
    with pytest.raises(_lib.VmapStepError):
        odometry.DepthTracker((10, 10, 4, 4), 2048, 1024, (2,))                           # past 2^20 pixels: refused at construction
    with pytest.raises(_lib.VmapStepError):
        odometry.DepthTracker((10, 10, 4, 4), 8, 8, (2, 2, 2, 2, 2))
    if not torch.cuda.is_available():                                                     # without a device: an error, never a fallback
        with pytest.raises(_lib.VmapStepError):
            odometry.depth_maps(np.ones((8, 8), f32), (10, 10, 4, 4), levels=1, min_depth=0.1, max_depth=10.0, band=0.1)
