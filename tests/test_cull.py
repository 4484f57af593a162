"""CPU tier of visibility culling: the numpy checker (tests/cull_oracle.py) in its two layers against each other, csrc/cull_rules.h -
compiled into the host program tests/tools/cull_rules_host.cpp with the address and undefined-behaviour sanitizers - against the
float32 layer bit for bit, the deliberate boundary cases of the contract with their answers written out, the known-answer scene, and
the argument checks of vmapstep_cull_* (no device is touched).  Nothing is held against an outside implementation: the contract of
include/vmapstep.h is this project's own."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import cull_cases as cc
import cull_oracle as co
from conftest import ROOT
from vmap_amd import _lib

f32 = np.float32


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """A stand-alone program with its own main, built with -fsanitize=address,undefined: any out-of-bounds access or undefined
    arithmetic in the rules aborts it."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("cull_host") / "cull_rules_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vmap_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "cull_rules_host.cpp"), "-o", exe], check=True)
    return exe


def hexes(a):
    return " ".join(f"{x:08x}" for x in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32).tolist())


def run_host(exe, tmp_path, points, depth, t_wc, intrinsics, width, height, eps=None, margin=0, min_depth=0.0):
    t_wc = np.asarray(t_wc, np.float32).reshape(-1, 4, 4)
    points = np.asarray(points, np.float32).reshape(-1, 3)
    assert eps is None or np.shape(depth) == (len(t_wc), width, height)
    lines = [hexes(list(intrinsics) + [min_depth, 0.0 if eps is None else eps]),
             f"{width} {height} {margin} {int(eps is not None)} {len(t_wc)} {len(points)}", hexes(t_wc[:, :3, :])]
    if eps is not None:
        lines.append(hexes(depth))
    lines.append(hexes(points))
    path = tmp_path / "scene.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.strip()
    assert len(out) == len(points)
    return np.array([int(ch) for ch in out], np.uint8)


SCENES = [(37, 23, 900, 5, 0.02, 0, 0.0), (64, 48, 900, 6, 0.05, 3, 0.5), (37, 23, 700, 4, None, 0, 0.0), (64, 48, 700, 3, None, 5, 1.0)]


@pytest.mark.parametrize("width,height,n,K,eps,margin,min_depth", SCENES)
def test_host_program_equals_the_float32_checker(host_exe, tmp_path, width, height, n, K, eps, margin, min_depth):
    """Random scenes with real rotations, non-square images, both modes, a margin and a min_depth, two all-zero spare poses."""
    pts, depth, t_wc, intr = cc.random_scene(width, height, n, K, seed=width + K, spare_slots=2)
    pts[5] = [np.nan, 0.1, 0.2]
    pts[6] = [0.1, np.inf, 0.2]
    want = co.seen_f32(pts, depth, t_wc, intr, width, height, eps, margin, min_depth)
    got = run_host(host_exe, tmp_path, pts, depth, t_wc, intr, width, height, eps, margin, min_depth)
    assert np.array_equal(got, want)
    assert 0.05 < want.mean() < 0.95 and want[5] == 0 and want[6] == 0
    if eps is not None:                                           # the depth images decide something: the frustum alone sees more
        assert co.seen_f32(pts, depth, t_wc, intr, width, height, None, margin, min_depth).sum() > want.sum()


@pytest.mark.parametrize("width,height,n,K,eps,margin,min_depth", SCENES)
def test_float32_checker_agrees_with_the_geometry_outside_the_bands(width, height, n, K, eps, margin, min_depth):
    """Against float64: a point may be left out only when one of its decisions lies within a band of its boundary (the image edge or
    a rounding tie: cull_oracle.PIXEL_BAND; z = d + eps or z = min_depth: DEPTH_BAND), and at most 2 % of the points are."""
    pts, depth, t_wc, intr = cc.random_scene(width, height, n, K, seed=width + K, spare_slots=2)
    got = co.seen_f32(pts, depth, t_wc, intr, width, height, eps, margin, min_depth).astype(bool)
    want, amb = co.seen_f64(pts, depth, t_wc, intr, width, height, eps, margin, min_depth)
    print(f"left out: {amb.sum()} of {n} ({amb.mean():.4%})")
    assert amb.mean() <= 0.02
    assert np.array_equal(got[~amb], want[~amb])


# ---- the deliberate cases: identity pose, fx = fy = 8, cx = 18, cy = 11 on a 37 x 23 image; a point (x, y, 2) projects to
# ---- u = 4 x + 18, v = 4 y + 11 exactly, so halves and edges are hit exactly ----------------------------------------------------------
W, H, K4 = 37, 23, (8.0, 8.0, 18.0, 11.0)
IDENT = np.eye(4, dtype=np.float32)[None]


def at(u, v, z=2.0):
    return [(u - 18.0) * z / 8.0, (v - 11.0) * z / 8.0, z]


def check_cases(host_exe, tmp_path, cases, depth, eps, margin=0, min_depth=0.0, t_wc=IDENT):
    pts = np.array([c[0] for c in cases], np.float32)
    want = np.array([c[1] for c in cases], np.uint8)
    got = co.seen_f32(pts, depth, t_wc, K4, W, H, eps, margin, min_depth)
    assert np.array_equal(got, want), [(c, g) for c, g in zip(cases, got) if g != c[1]]
    assert np.array_equal(run_host(host_exe, tmp_path, pts, depth, t_wc, K4, W, H, eps, margin, min_depth), want)
    return pts, want


def test_projection_on_a_half_rounds_to_even_in_both_directions(host_exe, tmp_path):
    """The depth image is 0 on odd columns / rows around the ties, so half-up or half-down rounding would give other answers."""
    depth = np.full((1, W, H), 5.0, np.float32)
    depth[0, 19, :] = 0.0                                         # 18.5 -> 18 (down to even), 19.5 -> 20 (up to even)
    depth[0, :, 7] = 0.0                                          # 6.5 -> 6, 7.5 -> 8
    cases = [(at(18.5, 3), 1), (at(19.5, 3), 1), (at(19.0, 3), 0), (at(19.25, 3), 0), (at(5, 6.5), 1), (at(5, 7.5), 1), (at(5, 7.0), 0),
             (at(18.5, 7.5), 1), (at(19.5, 6.5), 1)]
    check_cases(host_exe, tmp_path, cases, depth, 0.1)


def test_depth_boundaries(host_exe, tmp_path):
    """z == d + eps exactly is seen, one ulp beyond is not; z == 0 and z < 0; d == 0 is no measurement; a NaN coordinate or depth."""
    depth = np.full((1, W, H), 1.5, np.float32)
    depth[0, 4, 4] = 0.0
    depth[0, 6, 6] = np.nan
    depth[0, 8, 8] = -1.0
    up = float(np.nextafter(f32(2.0), f32(3.0)))
    cases = [(at(10, 10, 2.0), 1), (at(10, 10, up), 0), (at(10, 10, 1.0), 1), ([0.0, 0.0, 0.0], 0), ([0.0, 0.0, -0.0], 0), (at(10, 10, -2.0), 0),
             ([0.1, 0.1, -1.0], 0), (at(4, 4, 1.0), 0), (at(6, 6, 1.0), 0), (at(8, 8, 1.0), 0), ([np.nan, 0.0, 2.0], 0), ([0.0, np.nan, 2.0], 0),
             ([0.0, 0.0, np.nan], 0), ([np.inf, 0.0, 2.0], 0), ([0.0, 0.0, np.inf], 0)]
    pts, _ = check_cases(host_exe, tmp_path, cases, depth, 0.5)
    # frustum only: the depth image is not read - the hole, the NaN and the negative depth do not matter
    frustum = co.seen_f32(pts, None, IDENT, K4, W, H, None)
    assert frustum.tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert np.array_equal(run_host(host_exe, tmp_path, pts, None, IDENT, K4, W, H, None), frustum)
    # z == min_depth is not in front
    check_cases(host_exe, tmp_path, [(at(10, 10, 1.0), 0), (at(10, 10, float(np.nextafter(f32(1.0), f32(2.0)))), 1)], depth, None, 0, 1.0)


def test_image_edges_and_margin(host_exe, tmp_path):
    """w and h exactly at margin and at W - 1 - margin / H - 1 - margin, one pixel beyond, and the ties next to the edges."""
    depth = np.full((1, W, H), 5.0, np.float32)
    for margin in (0, 2):
        lo, whi, hhi = margin, W - 1 - margin, H - 1 - margin
        cases = [(at(lo, 10), 1), (at(lo - 1, 10), 0), (at(whi, 10), 1), (at(whi + 1, 10), 0), (at(10, lo), 1), (at(10, lo - 1), 0), (at(10, hhi), 1),
                 (at(10, hhi + 1), 0), (at(lo, lo), 1), (at(whi, hhi), 1), (at(lo - 0.25, 10), 1), (at(whi + 0.25, 10), 1), (at(lo - 0.75, 10), 0),
                 # the ties at the edges: lo - 0.5 rounds to even, whi + 0.5 too
                 (at(lo - 0.5, 10), int((lo - 1) % 2 == 1)), (at(whi + 0.5, 10), int(whi % 2 == 0)), (at(10, hhi + 0.5), int(hhi % 2 == 0))]
        for eps in (0.1, None):
            check_cases(host_exe, tmp_path, cases, depth, eps, margin)


def test_an_all_zero_pose_sees_nothing_and_a_rotated_pose_sees_what_it_faces(host_exe, tmp_path):
    depth = np.full((1, W, H), 5.0, np.float32)
    pts = [at(u, v) for u in range(0, W, 4) for v in range(0, H, 3)]
    zero = np.zeros((1, 4, 4), np.float32)
    check_cases(host_exe, tmp_path, [(p, 0) for p in pts], depth, 0.1, t_wc=zero)
    check_cases(host_exe, tmp_path, [(p, 0) for p in pts], depth, None, t_wc=zero)
    # a camera at (3, 0, 2) turned by 90 degrees about y looks along -x... its optical axis is R e_z
    R = cc.rotation([0, 1, 0], -np.pi / 2)
    T = cc.pose(R, [3.0, 0.0, 2.0])[None]
    ahead = (np.array([3.0, 0.0, 2.0]) + 2.0 * (R @ [0.1, -0.2, 1.0])).tolist()
    behind = (np.array([3.0, 0.0, 2.0]) - 2.0 * (R @ [0.1, -0.2, 1.0])).tolist()
    check_cases(host_exe, tmp_path, [(ahead, 1), (behind, 0)], depth, 0.1, t_wc=T)
    # width-major: a point far along the long side (u = 30) exists only if the image is read [W, H]
    d = np.zeros((1, W, H), np.float32)
    d[0, 30, 2] = 5.0
    check_cases(host_exe, tmp_path, [(at(30, 2), 1), (at(2, 30 - 8), 0)], d, 0.1)


def test_known_answer_scene(host_exe, tmp_path):
    """A wall and a box behind it: with the depth images every box vertex is unseen and the wall's vertices inside a frustum are
    seen; with the frustum alone the box is seen too; culling with occlusion leaves only wall faces."""
    s = cc.known_answer_scene()
    v, nw = s["vertices"], s["n_wall"]
    occl = co.seen_f32(v, s["depth"], s["t_wc"], cc.KA_INTRINSICS, cc.KA_W, cc.KA_H, cc.KA_EPS)
    frus = co.seen_f32(v, None, s["t_wc"], cc.KA_INTRINSICS, cc.KA_W, cc.KA_H, None)
    geo, amb = co.seen_f64(v, None, s["t_wc"], cc.KA_INTRINSICS, cc.KA_W, cc.KA_H, None)
    assert not amb.any()
    assert not occl[nw:].any() and frus[nw:].all()
    assert np.array_equal(occl[:nw].astype(bool), geo[:nw]) and np.array_equal(frus[:nw].astype(bool), geo[:nw])
    assert 10 < geo[:nw].sum() < nw - 100                         # part of the wall lies outside every frustum
    assert np.array_equal(run_host(host_exe, tmp_path, v, s["depth"], s["t_wc"], cc.KA_INTRINSICS, cc.KA_W, cc.KA_H, cc.KA_EPS), occl)
    faces, kept = co.cull_faces(s["faces"], occl, 1)
    assert len(faces) > 0 and kept.max() < nw
    assert len(co.cull_faces(s["faces"], frus, 3)[0]) >= 12      # the whole box survives the frustum test


def test_compaction_checker_on_a_hand_made_mesh():
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 4, 5], [5, 6, 0], [3, 3, 3]], np.int32)
    seen = np.array([1, 0, 0, 0, 1, 0, 0], np.uint8)
    f1, k1 = co.cull_faces(faces, seen, 1)
    assert k1.tolist() == [0, 1, 2, 3, 4, 5, 6] and f1.tolist() == [[0, 1, 2], [2, 3, 4], [4, 4, 5], [5, 6, 0]]
    f2, k2 = co.cull_faces(faces, seen, 2)                        # the repeated index counts once per corner
    assert k2.tolist() == [4, 5] and f2.tolist() == [[0, 0, 1]]
    f3, k3 = co.cull_faces(faces, seen, 3)
    assert len(f3) == 0 and len(k3) == 0                          # nothing kept
    fa, ka = co.cull_faces(faces, np.ones(7, np.uint8), 3)
    assert np.array_equal(fa, faces) and ka.tolist() == list(range(7))      # everything kept


# ---- the C ABI's argument checks ------------------------------------------------------------------------------------------------------

def _cfg(**kw):
    d = dict(fx=60.0, fy=60.0, cx=18.0, cy=11.0, min_depth=0.0, occlusion_eps=0.05, width=37, height=23, margin=0, use_depth=1)
    d.update(kw)
    return _lib.CullCfg(**d)


def test_abi_refuses_bad_arguments_before_anything_is_enqueued():
    """Every rejected argument of the cull section returns VMAPSTEP_ERR_ARGUMENT (-1) with a message, a short workspace -3; none of
    the calls reads a pointer or touches a device."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    ref = ctypes.byref
    mark = lambda cfg, n=5, k=2, depth=p, points=p, seen=p: lib.vmapstep_cull_mark(points, n, depth, p, None, k, cfg, seen, None)
    bad = (dict(width=0), dict(height=0), dict(width=-3), dict(margin=-1), dict(margin=12), dict(margin=19), dict(min_depth=-0.5),
           dict(min_depth=float("nan")), dict(occlusion_eps=-1e-3), dict(occlusion_eps=float("nan")), dict(fx=0.0), dict(cy=float("inf")))
    for kw in bad:
        assert mark(ref(_cfg(**kw))) == -1 and lib.vmapstep_last_error().startswith(b"cull"), kw
    assert mark(None) == -1
    assert mark(ref(_cfg()), depth=None) == -1 and b"null depth" in lib.vmapstep_last_error()
    assert mark(ref(_cfg()), n=-1) == -1 and mark(ref(_cfg()), k=-1) == -1 and mark(ref(_cfg()), n=1 << 31) == -1
    assert mark(ref(_cfg()), points=None) == -1 and mark(ref(_cfg()), seen=None) == -1
    # nothing to do is OK and touches nothing (the pointers are not even looked at); frustum only takes a null depth and any eps
    assert mark(ref(_cfg()), n=0) == 0 and mark(ref(_cfg()), k=0) == 0 and mark(ref(_cfg()), n=0, points=None, seen=None) == 0
    assert mark(ref(_cfg(use_depth=0, occlusion_eps=float("nan"))), depth=None, k=0) == 0
    assert mark(ref(_cfg(margin=11)), k=0) == 0                   # one row of pixels is left

    n = ctypes.c_size_t()
    assert lib.vmapstep_cull_workspace_bytes(100, 200, ref(n)) == 0 and n.value >= 100 + 400 + 16
    need = n.value
    assert lib.vmapstep_cull_workspace_bytes(100, 200, None) == -1 and lib.vmapstep_cull_workspace_bytes(-1, 200, ref(n)) == -1
    assert lib.vmapstep_cull_workspace_bytes(100, 1 << 31, ref(n)) == -1
    count = lambda min_seen=1, nf=200, nv=100, faces=p, seen=p, counts=p, ws=p, nb=need: \
        lib.vmapstep_cull_faces_count(faces, nf, seen, nv, min_seen, counts, ws, nb, None)
    emit = lambda min_seen=1, nf=200, nv=100, faces=p, kept=p, nkv=10, out=p, nkf=10, ws=p, nb=need: \
        lib.vmapstep_cull_faces_emit(faces, nf, p, nv, min_seen, kept, nkv, out, nkf, ws, nb, None)
    for ms in (0, 4, -1):
        assert count(ms) == -1 and emit(ms) == -1 and b"min_seen" in lib.vmapstep_last_error(), ms
    assert count(nf=-1) == -1 and count(nv=-1) == -1 and count(nv=1 << 31) == -1 and count(nv=0) == -1 and emit(nv=0) == -1
    assert count(faces=None) == -1 and count(seen=None) == -1 and count(counts=None) == -1
    assert emit(faces=None) == -1 and emit(kept=None) == -1 and emit(out=None) == -1 and emit(nkv=-1) == -1 and emit(nkf=-1) == -1
    assert count(nb=need - 1) == -3 and emit(nb=need - 1) == -3 and count(ws=p + 8) == -3 and b"cull workspace" in lib.vmapstep_last_error()
    assert emit(nkf=0, nkv=0, kept=None, out=None) == 0           # nothing to emit: nothing enqueued
    assert lib.vmapstep_abi_version() == 7


def test_cull_cfg_layout_matches_the_header(tmp_path):
    """The ctypes mirror of vmapstep_cull_cfg against include/vmapstep.h as gcc lays it out."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = [f for f, _ in _lib.CullCfg._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmapstep.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(vmapstep_cull_cfg));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(vmapstep_cull_cfg, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: int(l.split()[1]) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert got["size"] == ctypes.sizeof(_lib.CullCfg)
    for f in fields:
        assert got[f] == getattr(_lib.CullCfg, f).offset, f


def test_python_layer_refuses_what_it_can_before_the_library():
    from vmap_amd import visibility
    assert set(visibility.__all__) == {"mark_visible", "mark_visible_store", "cull_mesh", "cull_to_views"}
    import vmap_amd
    assert "visibility" in vmap_amd.__all__
    import torch
    with pytest.raises(_lib.VmapStepError):
        visibility._slots([0, 3], 3, "cpu")
    with pytest.raises(_lib.VmapStepError):
        visibility._slots(torch.tensor([-1]), 3, "cpu")
    sl, k = visibility._slots([2, 0], 3, "cpu")
    assert sl.dtype == torch.int32 and sl.tolist() == [2, 0] and k == 2 and visibility._slots(None, 7, "cpu") == (None, 7)
