"""CPU tier of the TSDF ray cast: csrc/raycast_rules.h - compiled into the stand-alone host program tests/tools/raycast_rules_host.cpp
with the address and undefined-behaviour sanitizers - against the exact layer of the numpy checker (tests/raycast_oracle.py) bit for bit
on every branch of the contract and on the scenes; the class-aware march against the plain one bit for bit, in both; the checker's
geometry and normals on the analytic corner-and-sphere scene; and the argument checks of the raycast entries of the C ABI (no device is
touched).  Nothing is held against an outside implementation: the contract of include/vmapstep.h is this project's own."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_cases as ic
import icp_oracle as io
import raycast_cases as rcs
import raycast_oracle as ro
import tsdf_cases as tc
from conftest import ROOT
from vmap_amd import _lib

f32 = np.float32


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """A stand-alone program with its own main, built with -fsanitize=address,undefined."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("raycast_host") / "raycast_rules_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vmap_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "raycast_rules_host.cpp"), "-o", exe], check=True)
    return exe


def run_host(exe, tmp_path, shape, vol, M, N, intr, width, height, **kw):
    (tmp_path / "in.bin").write_bytes(rcs.pack_host_input(shape, vol, M.astype(f32), N.astype(f32), intr, width, height, **kw))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    return rcs.unpack_host_output((tmp_path / "out.bin").read_bytes(), shape, len(M), width, height, vol["color"] is not None)


def assert_all_equal(exe, tmp_path, shape, A, vol, poses, intr, width, height, **kw):
    """Host plain == host class-aware == checker plain == checker class-aware, and the class bytes; -> (the result, the classes)."""
    _, M, N = ro.compose(A, poses)
    color = vol["color"] is not None
    classes, plain, classed = run_host(exe, tmp_path, shape, vol, M, N, intr, width, height, **kw)
    want_classes = ro.brick_classes(vol, shape, kw["min_weight"])
    assert np.array_equal(classes, want_classes)
    want = ro.raycast(vol, shape, M, N, intr, width, height, exact=True, bricks=None, color=color, **kw)
    want_classed = ro.raycast(vol, shape, M, N, intr, width, height, exact=True, bricks=want_classes, color=color, **kw)
    assert rcs.same_bits(plain, classed) == [] and rcs.same_bits(want, want_classed) == [] and rcs.same_bits(plain, want) == []
    return want, want_classes


# ---- every branch, by hand: a 26 x 3 x 3 line of voxels of 0.125 m whose index i runs along the optical axis of an identity camera --------
# world x = 0.125 j - 0.125, y = 0.125 k - 0.125, z = 0.125 i + 0.5: the centre pixel (2, 1) looks along i through j = k = 1 with
# d = (8, 0, 0) - parallel to two axes - and a sample every half voxel (step 0.0625: every number here is exact in binary)
LINE_SHAPE = (26, 3, 3)
LINE_AFFINE = np.array([[0, 0.125, 0, -0.125], [0, 0, 0.125, -0.125], [0.125, 0, 0, 0.5]])
LINE_INTR, LINE_W, LINE_H, CW, CH = (16.0, 16.0, 2.0, 1.0), 5, 3, 2, 1
LINE_KW = dict(min_depth=0.25, max_depth=10.0, min_weight=1.0, step=0.0625, max_steps=200)


def shifted(x=0.0, z=0.0):
    T = np.eye(4)
    T[0, 3], T[2, 3] = x, z
    return T


LINE_POSES = np.stack([np.eye(4), shifted(x=1.0), np.zeros((4, 4)), shifted(z=1.0)])    # identity; parallel and outside; unused; inside


def line_volume(profile, weight=None, wc=1.0):
    """tsdf = profile(i) for every (j, k); weight 1 (or weight(i, j, k)); colour (10 i, 100, 200) with colour weight wc(i, j, k)."""
    i, j, k = np.meshgrid(*[np.arange(s) for s in LINE_SHAPE], indexing="ij")
    D = np.vectorize(profile)(i).astype(f32)
    W = np.ones(LINE_SHAPE, f32) if weight is None else np.vectorize(weight)(i, j, k).astype(f32)
    wcs = np.full(LINE_SHAPE, wc, f32) if np.isscalar(wc) else np.vectorize(wc)(i, j, k).astype(f32)
    C = np.stack([10.0 * i, np.full(LINE_SHAPE, 100.0), np.full(LINE_SHAPE, 200.0), wcs], -1).astype(f32)
    return dict(tsdf=D.reshape(-1), weight=W.reshape(-1), color=C.reshape(-1, 4))


def ramp(i):                                  # 1.0 up to i = 10, zero at i = 12.5, -1 from i = 15
    return float(np.clip((12.5 - i) / 2, -1, 1))


def line(host_exe, tmp_path, vol, **kw):
    return assert_all_equal(host_exe, tmp_path, LINE_SHAPE, LINE_AFFINE, vol, LINE_POSES, LINE_INTR, LINE_W, LINE_H, **dict(LINE_KW, **kw))


def test_hit_miss_inside_parallel_and_unused_views(host_exe, tmp_path):
    got, classes = line(host_exe, tmp_path, line_volume(ramp))
    # the identity view: the crossing at i = 12.5 is at z = 0.5 + 0.125 * 12.5, the normal looks back along the optical axis
    assert got["status"][0, CW, CH] == ro.HIT and got["depth"][0, CW, CH] == f32(2.0625)
    assert np.array_equal(got["normal"][0, CW, CH], np.array([0, 0, -1], f32))
    assert np.array_equal(got["color"][0, CW, CH], [125, 100, 200, 255])              # the lerp of 120 and 130 at t = 0.5
    # its neighbours leave through the line's sides (j = 1 +- 0.5 z) before the crossing: no hit
    assert got["status"][0, CW + 1, CH] == ro.LEFT and got["depth"][0, CW + 1, CH] == 0
    # parallel to the j and k axes and outside on j: the zero-component branch; the other pixels of that view never reach the line
    assert (got["status"][1] == ro.MISS).all() and not got["depth"][1].any()
    # an unused slot; and an eye that starts inside the volume, at i = 4
    assert (got["status"][2] == ro.MISS).all() and not got["normal"][2].any() and not got["color"][2].any()
    assert got["status"][3, CW, CH] == ro.HIT and got["depth"][3, CW, CH] == f32(1.0625)
    # voxels 0 .. 8 are exactly 1.0 and valid: the first brick is FREE and the centre ray crosses it; the others are mixed
    assert classes[0, 0, 0] == ro.FREE and (classes[1:] == ro.MIXED).all()


def test_an_empty_brick_is_crossed_and_a_hole_stops_a_hit(host_exe, tmp_path):
    got, classes = line(host_exe, tmp_path, line_volume(ramp, weight=lambda i, j, k: float(i > 8)))
    assert classes[0, 0, 0] == ro.EMPTY and got["status"][0, CW, CH] == ro.HIT and got["depth"][0, CW, CH] == f32(2.0625)
    # positive up to i = 10, unobserved at 11 and 12, negative from 13: the invalid samples clear the state, the next valid one is behind
    hole = line_volume(lambda i: 1.0 if i <= 12 else -0.5, weight=lambda i, j, k: float(i not in (11, 12)))
    got, _ = line(host_exe, tmp_path, hole)
    assert got["status"][0, CW, CH] == ro.BEHIND and got["depth"][0, CW, CH] == 0 and not got["normal"][0, CW, CH].any()


def test_back_face_zero_and_the_step_limit(host_exe, tmp_path):
    got, _ = line(host_exe, tmp_path, line_volume(lambda i: -0.5))
    assert got["status"][0, CW, CH] == ro.BEHIND                                      # a back face first
    got, _ = line(host_exe, tmp_path, line_volume(lambda i: 0.0))
    assert got["status"][0, CW, CH] == ro.LEFT                                        # f == 0 without state: the ray goes on, and leaves
    got, _ = line(host_exe, tmp_path, line_volume(lambda i: 1.0 if i < 5 else 0.0))
    assert got["status"][0, CW, CH] == ro.HIT and got["depth"][0, CW, CH] == f32(0.5 + 0.125 * 5)    # f == 0 with the state set: a hit there
    # all free space: 51 samples (i = 0, 0.5 .. 25) fit the range; the 52nd is past it.  max_steps 51 leaves, 50 runs out.
    free = line_volume(lambda i: 1.0)
    assert line(host_exe, tmp_path, free)[0]["status"][0, CW, CH] == ro.LEFT
    assert line(host_exe, tmp_path, free, max_steps=51)[0]["status"][0, CW, CH] == ro.LEFT
    got, classes = line(host_exe, tmp_path, free, max_steps=50)
    assert got["status"][0, CW, CH] == ro.STEPS and got["depth"][0, CW, CH] == 0 and (classes == ro.FREE).all()
    assert line(host_exe, tmp_path, free, max_steps=7)[0]["status"][0, CW, CH] == ro.STEPS


def test_a_hit_in_the_last_cell(host_exe, tmp_path):
    """The sample at p = n - 1 = 25 is taken in cell 24 at t = 1: 3 at voxel 24 and -1 at voxel 25 give f(24.5) = 1, f(25) = -1."""
    got, _ = line(host_exe, tmp_path, line_volume(lambda i: 1.0 if i < 24 else 3.0 if i == 24 else -1.0))
    assert got["status"][0, CW, CH] == ro.HIT and got["depth"][0, CW, CH] == f32(0.5 + 0.125 * 24.75)


def test_normal_refused_and_colour_with_some_and_no_coloured_corners(host_exe, tmp_path):
    # voxel (14, 2, 2) unobserved: the march hits at i = 12.5 before it reaches the cell, the normal's sample at i = 13.5 does not
    got, _ = line(host_exe, tmp_path, line_volume(ramp, weight=lambda i, j, k: float((i, j, k) != (14, 2, 2))))
    assert got["status"][0, CW, CH] == ro.HIT and got["depth"][0, CW, CH] == f32(2.0625) and not got["normal"][0, CW, CH].any()
    assert got["color"][0, CW, CH, 3] == 255
    # one coloured corner out of eight, of trilinear weight 0.5: renormalised, the pixel is that voxel's colour
    got, _ = line(host_exe, tmp_path, line_volume(ramp, wc=lambda i, j, k: float((i, j, k) == (12, 1, 1))))
    assert np.array_equal(got["color"][0, CW, CH], [120, 100, 200, 255])
    got, _ = line(host_exe, tmp_path, line_volume(ramp, wc=0.0))
    assert got["status"][0, CW, CH] == ro.HIT and not got["color"].any()


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", rcs.IMAGES)
@pytest.mark.parametrize("state", rcs.STATES)
@pytest.mark.parametrize("name", list(rcs.SHAPES))
def test_host_equals_the_exact_checker_on_the_scenes(host_exe, tmp_path, name, state, width, height):
    vol, shape, A = rcs.volume(name, state)
    poses, intr = rcs.views_of(shape, A), ic.intrinsics_for(width, height)
    got, classes = assert_all_equal(host_exe, tmp_path, shape, A, vol, poses, intr, width, height, **rcs.KW)
    assert (got["status"][1] == ro.MISS).all() and (got["status"][0] != ro.MISS).any() and (got["status"][2] != ro.MISS).any()
    if name == "19x26x33":
        assert (got["status"] == ro.HIT).any() and (got["status"] == ro.LEFT).any() and (got["status"] == ro.BEHIND).any()
        if state == "fused":
            assert (classes == ro.EMPTY).any() and (classes == ro.FREE).any() and (classes == ro.MIXED).any()
    # K views in one call == the same views one at a time, in the checker and in the host program
    _, M, N = ro.compose(A, poses)
    for k in range(len(poses)):
        one = ro.raycast(vol, shape, M[k:k + 1], N, intr, width, height, exact=True, bricks=classes, color=True, **rcs.KW)
        assert rcs.same_bits({key: got[key][k:k + 1] for key in ("depth", "status", "normal", "color")}, one) == []
    if (width, height) == rcs.IMAGES[0]:
        _, plain, classed = run_host(host_exe, tmp_path, shape, vol, M[2:3], N, intr, width, height, **rcs.KW)
        assert rcs.same_bits({key: got[key][2:3] for key in ("depth", "status", "normal", "color")}, plain) == [] and rcs.same_bits(plain, classed) == []


# ---- geometry and normals, on the checker alone -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cast():
    plain, exact, shape, A = rcs.geometry_volumes()
    intr = ic.intrinsics_for(tc.WIDTH, tc.HEIGHT)
    t32, M, N = ro.compose(A, np.stack([ic.look_at(e, tc.TARGET) for e in rcs.GEOMETRY_EYES]))
    return dict(plain=ro.raycast(plain, shape, M, N, intr, tc.WIDTH, tc.HEIGHT, exact=False, **rcs.GEOMETRY_KW),
                exact=ro.raycast(exact, shape, M, N, intr, tc.WIDTH, tc.HEIGHT, exact=True, **rcs.GEOMETRY_KW), t_wc=t32, intrinsics=intr,
                weight=plain["weight"].reshape(shape))


def test_geometry_of_the_analytic_scene(cast):
    W, H, (fx, fy, cx, cy) = tc.WIDTH, tc.HEIGHT, cast["intrinsics"]
    w, h = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    length = np.sqrt(((w - cx) / fx) ** 2 + ((h - cy) / fy) ** 2 + 1)
    for layer in ("plain", "exact"):
        for k in range(len(rcs.GEOMETRY_EYES)):
            truth = ic.render(cast["t_wc"][k].astype(np.float64), cast["intrinsics"], W, H)
            edge = rcs.edge_mask(truth)
            compared = (cast[layer]["status"][k] == ro.HIT) & ~edge
            err = np.abs(cast[layer]["depth"][k].astype(np.float64) - truth)[compared] * length[compared] / tc.VOXEL
            print(f"{layer} eye {k}: excluded {edge.mean():.4f}, compared {compared.mean():.4f}, beyond half a voxel {(err > 0.5).mean():.4f}, "
                  f"worst {err.max():.3f}, median {np.median(err):.3f} voxel")
            assert edge.mean() <= rcs.MAX_EXCLUDED and compared.mean() >= rcs.MIN_COMPARED
            assert (err > 0.5).mean() <= rcs.MAX_SHARE_BEYOND_HALF and err.max() <= rcs.MAX_WORST_VOXELS
            if layer == "plain":
                assert abs(edge.mean() - rcs.PLAIN_EXCLUDED[k]) < 1e-3 and abs(compared.mean() - rcs.PLAIN_COMPARED[k]) < 1e-3
                assert abs((err > 0.5).mean() - rcs.PLAIN_SHARE_BEYOND_HALF[k]) < 1e-3 and abs(err.max() - rcs.PLAIN_WORST_VOXELS[k]) < 5e-3
    # the two layers: the same pixels hit, depths within twice the measured difference
    assert np.array_equal(cast["plain"]["status"], cast["exact"]["status"])
    diff = np.abs(cast["plain"]["depth"] - cast["exact"]["depth"].astype(np.float64)).max()
    print(f"exact against plain: {diff:.4e} m")
    assert rcs.EXACT_PLAIN_MAX_DIFF / 2 <= diff <= 2 * rcs.EXACT_PLAIN_MAX_DIFF


def near_invalid(weight, min_weight, reach):
    """bool, the volume padded by one voxel: True within `reach` voxels (Chebyshev) of a voxel below min_weight or of the padding."""
    m = np.pad(weight < min_weight, 1, constant_values=True)
    for _ in range(reach):
        for ax in range(3):
            lo, hi = np.roll(m, 1, ax), np.roll(m, -1, ax)          # the wrap-around meets the padding, which is True anyway
            m = m | lo | hi
    return m


@pytest.mark.parametrize("layer", ["plain", "exact"])
def test_normals_of_the_checker(cast, layer):
    res = cast[layer]
    hit = res["status"] == ro.HIT
    p = ro.hit_points_world(res, cast["t_wc"], cast["intrinsics"])[hit]
    n = res["normal"][hit].astype(np.float64)
    out, refused = tc.excluded(p), ~n.any(1)
    dots = (n * tc.outward(p)).sum(1)[~out & ~refused]
    print(f"{layer}: {100 * out.mean():.2f} % of the hits excluded by the one-voxel rule, {100 * refused.mean():.2f} % refused, smallest dot {dots.min():.4f}")
    assert abs(out.mean() - rcs.NORMALS_EXCLUDED_SHARE) < 2e-3 and out.mean() < tc.MAX_EXCLUDED_SHARE
    assert dots.min() >= tc.MIN_DOT_OUTSIDE_RULE and abs(dots.min() - rcs.PLAIN_MIN_DOT) < 5e-3
    assert np.abs(np.linalg.norm(n[~refused], axis=1) - 1).max() < 1e-6
    # a refused normal is a hit next to what no frame observed or to the volume's faces: each one, and their share
    assert abs(refused.mean() - rcs.NORMALS_REFUSED_SHARE) < 2e-3 and refused.mean() <= 2 * rcs.NORMALS_REFUSED_SHARE
    idx = np.clip(np.rint((p[refused] - tc.LO) / tc.VOXEL).astype(int), 0, tc.GRID - 1) + 1
    assert near_invalid(cast["weight"], 1.0, rcs.REFUSED_REACH)[idx[:, 0], idx[:, 1], idx[:, 2]].all()


def test_tracker_converges_on_the_checkers_raycast():
    """The CPU path of DepthTracker.track_to_volume: the exact layer's depth image at the model pose, then icp_oracle.track."""
    _, exact, shape, A = rcs.geometry_volumes()
    sc, P = ic.corner_scene(64, 48), ic.PARAMS
    _, M, N = ro.compose(A, sc["t_wc_model"][None])
    model = ro.raycast(exact, shape, M, N, sc["intrinsics"], 64, 48, exact=True, normals=False,
                       **dict(rcs.GEOMETRY_KW, min_depth=P.min_depth, max_depth=P.max_depth))["depth"][0]
    res = io.track(sc["depth"], model, sc["T_init"], sc["intrinsics"], ic.ITERATIONS, P)
    factor = ic.INITIAL_ERROR / io.pose_error(res["pose"], sc["T_true"])
    print(f"the pose error falls by a factor {factor:.3f}")
    assert abs(factor - rcs.TRACK_FACTOR) <= 0.01 * rcs.TRACK_FACTOR


# ---- the C ABI's argument checks, without a device ------------------------------------------------------------------------------------
def cfg(**kw):
    base = dict(nx=8, ny=8, nz=8, width=64, height=48, max_steps=100, flags=0, reserved=0, fx=60.0, fy=60.0, cx=31.5, cy=23.5, min_depth=0.0,
                max_depth=10.0, step=0.05, min_weight=1.0, normal_map=(ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), reserved_f=0.0)
    base.update(kw)
    return _lib.RaycastCfg(**base)


def test_struct_layout_matches_the_header(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    fields = ("width", "max_steps", "flags", "fx", "min_depth", "step", "min_weight", "normal_map", "reserved_f")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "vmapstep.h"\nint main() { std::printf("%zu' + " %zu" * len(fields) + '\\n", '
                   "sizeof(vmapstep_raycast_cfg), " + ", ".join(f"offsetof(vmapstep_raycast_cfg, {f})" for f in fields) + "); }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    C = _lib.RaycastCfg
    assert got == [ctypes.sizeof(C)] + [getattr(C, f).offset for f in fields]


def test_raycast_entry_checks_its_arguments_without_a_device():
    lib = _lib.load()
    assert all(e in _lib.EXPORTS for e in ("vmapstep_tsdf_bricks_bytes", "vmapstep_tsdf_bricks", "vmapstep_tsdf_raycast"))
    buf = ctypes.create_string_buffer(2048)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    call = lambda c, tsdf=p, weight=p, color=None, bricks=None, views=p, n=0, depth=p, status=p, normal=None, color_out=None: \
        lib.vmapstep_tsdf_raycast(None if c is None else ctypes.byref(c), tsdf, weight, color, bricks, views, n, depth, status, normal, color_out, None)
    assert call(cfg()) == 0                                               # n_views == 0: nothing is enqueued
    assert call(cfg(), color=p, bricks=p, normal=p, color_out=p) == 0 and call(cfg(), status=p + 1) == 0
    assert call(None) == -1
    for name in ("tsdf", "weight", "views", "depth", "status"):
        assert call(cfg(), **{name: None}) == -1, name
    for name in ("tsdf", "weight", "views", "depth", "normal"):
        assert call(cfg(), **{name: p + 2}) == -1 and b"aligned" in lib.vmapstep_last_error(), name
    assert call(cfg(), color=p + 8) == -1 and call(cfg(), bricks=p + 4) == -1 and call(cfg(), color=p, color_out=p + 2) == -1
    assert call(cfg(), color_out=p) == -1 and b"colour volume" in lib.vmapstep_last_error()
    nan, inf = float("nan"), float("inf")
    for kw in (dict(step=0.0), dict(step=-1.0), dict(step=nan), dict(step=inf), dict(min_weight=0.0), dict(min_weight=nan), dict(min_weight=inf),
               dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(fy=inf), dict(cx=nan), dict(cy=inf), dict(min_depth=-1.0), dict(min_depth=nan),
               dict(max_depth=0.0), dict(min_depth=2.0, max_depth=1.0), dict(max_depth=nan), dict(max_steps=0), dict(max_steps=-1),
               dict(max_steps=1 << 24), dict(width=0), dict(height=0), dict(width=1 << 15, height=1 << 15),
               dict(normal_map=(ctypes.c_float * 9)(*([nan] * 9)))):
        assert call(cfg(**kw)) == -1, kw
    assert call(cfg(max_steps=(1 << 24) - 1)) == 0 and call(cfg(max_depth=inf)) == 0
    assert call(cfg(), n=-1) == -1
    assert call(cfg(nx=1)) == -2 and call(cfg(nx=1024, ny=1024, nz=1024)) == -2               # the mesh section's limits
    assert call(cfg(nx=894, ny=894, nz=895)) == 0 and call(cfg(nx=895, ny=895, nz=894)) == -2


def test_bricks_entries_check_their_arguments_without_a_device():
    lib = _lib.load()
    nb = ctypes.c_size_t()
    assert lib.vmapstep_tsdf_bricks_bytes(8, 8, 8, None) == -1
    assert lib.vmapstep_tsdf_bricks_bytes(1, 8, 8, ctypes.byref(nb)) == -2
    for shape, want in (((2, 2, 2), 16), ((9, 9, 9), 16), ((10, 9, 9), 16), ((19, 26, 33), 48), ((256, 256, 256), 32768), ((258, 256, 256), 33 * 32 * 32)):
        assert lib.vmapstep_tsdf_bricks_bytes(*shape, ctypes.byref(nb)) == 0 and nb.value == want, shape
        assert int(np.prod([ro.brick_dim(s) for s in shape])) <= want < int(np.prod([ro.brick_dim(s) for s in shape])) + 16
    buf = ctypes.create_string_buffer(2048)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    call = lambda shape=(8, 8, 8), mw=1.0, tsdf=p, weight=p, bricks=p: lib.vmapstep_tsdf_bricks(*shape, mw, tsdf, weight, bricks, None)
    for name in ("tsdf", "weight", "bricks"):
        assert call(**{name: None}) == -1, name
    assert call(tsdf=p + 2) == -1 and call(weight=p + 1) == -1 and call(bricks=p + 8) == -1 and b"aligned" in lib.vmapstep_last_error()
    for mw in (0.0, -1.0, float("nan"), float("inf")):
        assert call(mw=mw) == -1, mw
    assert call(shape=(8, 8, 1)) == -2 and call(shape=(1024, 1024, 1024)) == -2


def test_volume_view_is_exported():
    import vmap_amd
    from vmap_amd import odometry, tsdf
    assert vmap_amd.VolumeView is tsdf.VolumeView and vmap_amd.TSDFVolume is tsdf.TSDFVolume
    assert hasattr(tsdf.TSDFVolume, "raycast") and hasattr(odometry.DepthTracker, "track_to_volume")
    assert (tsdf.VolumeView.MISS, tsdf.VolumeView.HIT, tsdf.VolumeView.LEFT, tsdf.VolumeView.BEHIND, tsdf.VolumeView.STEPS) == (0, 1, 2, 3, 4)
