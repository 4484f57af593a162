"""CPU tier of TSDF fusion: csrc/tsdf_rules.h - compiled into the stand-alone host program tests/tools/tsdf_rules_host.cpp with the
address and undefined-behaviour sanitizers - against the exact layer of the numpy checker (tests/tsdf_oracle.py) bit for bit on every
branch of the contract; the checker's geometry, normals and winding on the analytic corner-and-sphere scene; and the argument checks
of the tsdf and masked-mesh entries of the C ABI (no device is touched).  Nothing is held against an outside implementation: the
contract of include/vmapstep.h is this project's own."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_oracle as to
from conftest import ROOT
from vmap_amd import _lib

f32 = np.float32


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """A stand-alone program with its own main, built with -fsanitize=address,undefined."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("tsdf_host") / "tsdf_rules_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vmap_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "tsdf_rules_host.cpp"), "-o", exe], check=True)
    return exe


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def run_host(exe, tmp_path, shape, affine, sc, vol, **kw):
    color = vol["color"] is not None
    (tmp_path / "in.bin").write_bytes(tc.pack_host_input(shape, affine, sc, color=color, vol=vol, **kw))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    return tc.unpack_host_output((tmp_path / "out.bin").read_bytes(), int(np.prod(shape)), color)


def assert_host_equals_checker(exe, tmp_path, shape, affine, sc, vol, **kw):
    got = run_host(exe, tmp_path, shape, affine, sc, vol, **kw)
    want = to.integrate_f32(vol, shape, affine, sc["depth"], sc["t_wc"], sc["intrinsics"], rgbx=sc["rgbx"], inst=sc["inst"],
                            **{k: v for k, v in kw.items()})
    assert np.array_equal(bits(got["centres"]), bits(to.centers_f32(shape, affine)))
    for key in ("tsdf", "weight") + (("color",) if vol["color"] is not None else ()):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    return want


# ---- every branch, by hand: voxel i sits at (0.1 i, 0, 1) and lands on pixel (i, 1) of an identity camera with fx = 10 ---------------
N, TR, MAXD = 16, 0.25, 4.0
LINE_AFFINE = np.array([[0.1, 0, 0, 0.0], [0, 0.1, 0, 0.0], [0, 0, 0.1, 1.0]])
BELOW = float(np.nextafter(f32(0.75), f32(0)))
#             0: margin  1: fine  2: NaN   3: inf   4: -inf    5: 0  6: neg  7: == max  8: just above       9: sdf == -trunc
LINE_DEPTH = [1.0,       1.1,     np.nan,  np.inf,  -np.inf,   0.0,  -1.0,  MAXD,      float(np.nextafter(f32(MAXD), f32(9))), 0.75,
              # 10: one ulp below  11: clipped s, outside the band  12: other instance  13: inst -1  14: margin (w = width - 1)  15: outside
              BELOW,               3.0,                             1.1,                1.1,         1.1]


def line_scene():
    width, height = N - 1, 3                       # voxel 15 projects onto w = 15: outside the image; 0 and 14 inside the margin
    depth = np.zeros((4, width, height), f32)
    depth[0, :, 1] = np.array(LINE_DEPTH, f32)
    depth[1] = depth[0]                            # slot 1: the camera turned round, every voxel behind it
    depth[3] = depth[0]                            # slot 3: depth present, the pose all zero (an unused slot); slot 2: everything zero
    inst = np.full((4, width, height), 1, np.int32)
    inst[:, 12, 1], inst[:, 13, 1] = 2, -1
    t_wc = np.zeros((4, 4, 4), f32)
    t_wc[0] = np.eye(4)
    t_wc[1] = np.diag([-1.0, 1.0, -1.0, 1.0])
    rgbx = np.stack([tc.colour_image(width, height, k) for k in range(4)])
    return dict(depth=depth, t_wc=t_wc, intrinsics=(10.0, 10.0, 0.0, 1.0), inst=inst, rgbx=rgbx)


LINE_KW = dict(trunc=TR, max_weight=3.0, margin=1, min_depth=0.0, max_depth=MAXD)


@pytest.mark.parametrize("obj_id", [None, 1])
def test_host_equals_the_exact_checker_on_every_branch(host_exe, tmp_path, obj_id):
    shape, sc = (N, 1, 1), line_scene()
    vol = to.empty(shape, color=True)
    one = assert_host_equals_checker(host_exe, tmp_path, shape, LINE_AFFINE, sc, vol, obj_id=obj_id, slots=[0], **LINE_KW)
    updated = one["weight"] == 1
    want = {1, 7, 9, 11} | ({12, 13} if obj_id is None else set())
    # behind nothing, inside the image less the margin, a usable depth, the right instance, sdf >= -trunc: exactly these
    assert set(np.flatnonzero(updated)) == want and set(np.flatnonzero(one["weight"] == 0)) == set(range(N)) - want
    assert one["tsdf"][9] == -1.0 and one["tsdf"][11] == 1.0 and one["tsdf"][7] == 1.0            # sdf == -trunc updates; s clipped at 1
    assert one["tsdf"][1] == f32(f32(1.1) - f32(1)) / f32(TR)
    assert one["color"][1, 3] == 1 and one["color"][9, 3] == 1                                    # inside the band
    assert one["color"][11, 3] == 0 and one["color"][7, 3] == 0 and not one["color"][11, :3].any()  # outside: D and W move, the colour not
    assert np.array_equal(one["color"][1, :3], sc["rgbx"][0, 1, 1, :3].astype(f32))
    # behind the camera, a wholly empty slot and an all-zero pose with depth present: nothing moves
    for slot in (1, 2, 3):
        same = assert_host_equals_checker(host_exe, tmp_path, shape, LINE_AFFINE, sc, one, obj_id=obj_id, slots=[slot], **LINE_KW)
        for key in ("tsdf", "weight", "color"):
            assert np.array_equal(bits(same[key]), bits(one[key]))
    # the weight cap (3) reached at the third repetition and passed at the fourth and fifth, with frames that see nothing in between
    five = assert_host_equals_checker(host_exe, tmp_path, shape, LINE_AFFINE, sc, vol, obj_id=obj_id, slots=[0, 1, 0, 3, 0, 0, 2, 0], **LINE_KW)
    assert set(five["weight"][sorted(want)]) == {3.0} and five["color"][1, 3] == 3.0


CASES = [((8, 8, 8), "grid", 64, 48, 3), ((17, 13, 11), "grid", 37, 29, 5), ((5, 9, 70), "oriented", 64, 48, 4)]


def case_affine(shape, kind):
    if kind == "oriented":
        return tc.oriented_affine()
    s = 1.5 / (max(shape) - 1)
    return np.array([[s, 0, 0, tc.LO], [0, s, 0, tc.LO], [0, 0, s, tc.LO]])


@pytest.mark.parametrize("shape,kind,width,height,frames", CASES)
@pytest.mark.parametrize("obj_id", [None, tc.SPHERE_ID])
def test_host_equals_the_exact_checker_on_the_scenes(host_exe, tmp_path, shape, kind, width, height, frames, obj_id):
    """The corner scene with dirty depth, an unused slot among the frames, shuffled and repeated slots, a pre-filled colour volume and
    a cap of 3 that bites."""
    sc = tc.many_frames(width, height, frames, seed=width)
    A = case_affine(shape, kind)
    slots = list(np.random.default_rng(1).integers(0, frames, 2 * frames))
    want = assert_host_equals_checker(host_exe, tmp_path, shape, A, sc, tc.prefilled(shape, True, 3), obj_id=obj_id, slots=slots, trunc=0.2,
                                      max_weight=3.0, margin=1, min_depth=0.1, max_depth=tc.MAX_DEPTH)
    assert (want["weight"] == 3).any() and (want["weight"] < 3).any()


# ---- the checker itself on the analytic scene -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused():
    sc, shape, A = tc.scene(), (tc.GRID,) * 3, tc.grid_affine()
    kw = dict(trunc=tc.TRUNC, max_depth=tc.MAX_DEPTH)
    plain = to.integrate_f64(to.empty(shape, dtype=np.float64), shape, A, sc["depth"], sc["t_wc"], sc["intrinsics"], **kw)
    exact = to.integrate_f32(to.empty(shape), shape, A, sc["depth"], sc["t_wc"], sc["intrinsics"], **kw)
    return dict(plain=to.extract(plain, shape, A), exact=to.extract(exact, shape, A))


def test_geometry_of_the_analytic_scene(fused):
    pos, faces, _, edges, _ = fused["plain"]
    d = np.abs(tc.true_sdf(pos)) / tc.VOXEL
    print(f"plain layer: {len(pos)} vertices, {100 * (d > 0.5).mean():.2f} % beyond half a voxel, worst {d.max():.3f} voxel")
    assert len(pos) == tc.PLAIN_VERTICES and abs((d > 0.5).mean() - tc.PLAIN_SHARE_BEYOND_HALF) < 1e-4 and abs(d.max() - tc.PLAIN_WORST_VOXELS) < 5e-3
    assert len(pos) >= tc.MIN_VERTICES and (d > 0.5).mean() <= tc.MAX_SHARE_BEYOND_HALF and d.max() <= tc.MAX_WORST_VOXELS
    epos, efaces, _, eedges, _ = fused["exact"]
    de = np.abs(tc.true_sdf(epos)) / tc.VOXEL
    assert len(epos) >= tc.MIN_VERTICES and (de > 0.5).mean() <= tc.MAX_SHARE_BEYOND_HALF and de.max() <= tc.MAX_WORST_VOXELS
    # the two layers: the same edges carry a vertex, the same faces, coordinates within twice the measured difference
    assert np.array_equal(edges, eedges) and np.array_equal(faces, efaces)
    diff = np.abs(pos.astype(np.float64) - epos).max()
    print(f"exact against plain: {diff:.4e} m")
    assert diff <= 2 * tc.EXACT_PLAIN_MAX_DIFF and diff >= tc.EXACT_PLAIN_MAX_DIFF / 2


@pytest.mark.parametrize("layer", ["plain", "exact"])
def test_normals_and_winding_of_the_checker(fused, layer):
    pos, faces, nrm, _, _ = fused[layer]
    out = tc.excluded(pos)
    print(f"{layer}: {100 * out.mean():.2f} % of the vertices excluded by the one-voxel rule")
    assert abs(out.mean() - tc.EXCLUDED_SHARE) < 2e-3 and out.mean() < tc.MAX_EXCLUDED_SHARE
    dots = (nrm * tc.outward(pos)).sum(1)
    assert (dots[~out] > 0).all() and abs(dots[~out].min() - tc.MIN_DOT_OUTSIDE_RULE) < 5e-3
    fn = np.cross(pos[faces[:, 1]] - pos[faces[:, 0]], pos[faces[:, 2]] - pos[faces[:, 0]]).astype(np.float64)
    agree = (fn[:, None, :] * nrm[faces]).sum(-1)
    inside = ~out[faces].any(1)
    print(f"{layer}: {(agree <= 0).sum()} of {agree.size} corners disagree with their face, {(agree[inside] <= 0).sum()} outside the rule")
    assert (agree[inside] > 0).all()
    assert (agree <= 0).sum() == 8 and (agree <= 0).any(1).sum() == 4                    # tsdf_cases.py: the 90-degree creases
    assert len(np.unique(faces)) == len(pos) and np.isfinite(pos).all()                 # no vertex is unreferenced


def test_tracker_converges_on_the_checkers_mesh(fused):
    import icp_cases as ic
    import icp_oracle as io
    import raster_oracle as ro
    pos, faces, _, _, _ = fused["exact"]
    sc, P = ic.corner_scene(64, 48), ic.PARAMS
    model = ro.raster_f32(pos, faces, sc["t_wc_model"][None].astype(f32), sc["intrinsics"], 64, 48, P.min_depth)["depth"][0]
    res = io.track(sc["depth"], model, sc["T_init"], sc["intrinsics"], ic.ITERATIONS, P)
    factor = ic.INITIAL_ERROR / io.pose_error(res["pose"], sc["T_true"])
    print(f"the pose error falls by a factor {factor:.3f}")
    assert abs(factor - tc.TRACK_FACTOR) <= 0.01 * tc.TRACK_FACTOR


def test_masked_marching_cubes_of_the_checker():
    """All ones is the unmasked checker; all zeros is empty; random masks leave no vertex unreferenced and no invalid value in use."""
    import mesh_oracle as mo
    rng = np.random.default_rng(5)
    A = tc.oriented_affine()
    for seed in range(6):
        vol = rng.uniform(-1, 1, (9, 7, 5)).astype(f32)
        v, f, n, e = mo.marching_cubes(vol, 0.0, A)
        mv, mf, mn, me, _ = to.marching_cubes(vol, np.ones(vol.shape, bool), 0.0, A)
        assert np.array_equal(e, me) and np.array_equal(f, mf) and np.array_equal(bits(v), bits(mv)) and np.array_equal(bits(n), bits(mn))
        assert len(to.marching_cubes(vol, np.zeros(vol.shape, bool), 0.0, A)[0]) == 0
        valid = rng.uniform(size=vol.shape) < (0.95, 0.8, 0.6)[seed % 3]
        poisoned = np.where(valid, vol, np.nan).astype(f32)
        mv, mf, mn, me, _ = to.marching_cubes(poisoned, valid, 0.0, A)
        assert len(mf) and np.isfinite(mv).all() and np.isfinite(mn).all() and len(np.unique(mf)) == len(mv)
        assert set(me) <= set(e)


# ---- the C ABI's argument checks, without a device ------------------------------------------------------------------------------------
def cfg(**kw):
    base = dict(nx=8, ny=8, nz=8, obj_id=-1, affine=(ctypes.c_float * 12)(0.1, 0, 0, 0, 0, 0.1, 0, 0, 0, 0, 0.1, 0), fx=60.0, fy=60.0, cx=31.5,
                cy=23.5, width=64, height=48, margin=0, reserved=0, min_depth=0.0, max_depth=10.0, trunc=0.1, max_weight=64.0)
    base.update(kw)
    return _lib.TsdfCfg(**base)


def test_struct_layout_matches_the_header(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "vmapstep.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(vmapstep_tsdf_cfg), offsetof(vmapstep_tsdf_cfg, obj_id), offsetof(vmapstep_tsdf_cfg, affine), "
                   "offsetof(vmapstep_tsdf_cfg, fx), offsetof(vmapstep_tsdf_cfg, margin), offsetof(vmapstep_tsdf_cfg, max_weight)); }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    C = _lib.TsdfCfg
    assert got == [ctypes.sizeof(C), C.obj_id.offset, C.affine.offset, C.fx.offset, C.margin.offset, C.max_weight.offset]


def test_tsdf_entry_checks_its_arguments_without_a_device():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(2048)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    call = lambda c, tsdf=p, weight=p, color=None, depth=p, rgbx=None, inst=None, poses=p, slots=None, n=1: \
        lib.vmapstep_tsdf_integrate(None if c is None else ctypes.byref(c), tsdf, weight, color, depth, rgbx, inst, poses, slots, n, None)
    assert call(cfg(), n=0) == 0                                          # nothing to do: nothing is enqueued
    assert call(None) == -1
    for name in ("tsdf", "weight", "depth", "poses"):
        assert call(cfg(), **{name: None}) == -1, name
        assert call(cfg(), **{name: p + 2}) == -1 and b"aligned" in lib.vmapstep_last_error(), name
    assert call(cfg(), color=p + 8, rgbx=p) == -1 and call(cfg(), inst=p + 1, n=0) == -1 and call(cfg(), slots=p + 2, n=0) == -1
    assert call(cfg(), color=p, n=0) == -1 and b"rgbx" in lib.vmapstep_last_error()
    assert call(cfg(), color=p, rgbx=p, n=0) == 0
    assert call(cfg(obj_id=0), n=0) == -1 and b"inst" in lib.vmapstep_last_error()
    assert call(cfg(obj_id=0), inst=p, n=0) == 0
    for kw in (dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=float("nan")), dict(trunc=float("inf")), dict(max_weight=0.5),
               dict(max_weight=float("nan")), dict(max_depth=0.0), dict(min_depth=-1.0), dict(width=0), dict(margin=24), dict(fx=0.0),
               dict(affine=(ctypes.c_float * 12)(*([float("nan")] * 12)))):
        assert call(cfg(**kw), n=0) == -1, kw
    assert call(cfg(), n=-1) == -1
    assert call(cfg(nx=1), n=0) == -2 and call(cfg(nx=1024, ny=1024, nz=1024), n=0) == -2       # the mesh section's limits
    assert call(cfg(nx=894, ny=894, nz=895), n=0) == 0 and call(cfg(nx=895, ny=895, nz=894), n=0) == -2   # 3 n < 2^31


def test_masked_mesh_entries_check_their_arguments_without_a_device():
    lib = _lib.load()
    nb = ctypes.c_size_t()
    assert lib.vmapstep_mesh_workspace_bytes(8, 8, 8, ctypes.byref(nb)) == 0
    buf = ctypes.create_string_buffer(nb.value + 512)
    ws = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    vol = ctypes.addressof(ctypes.create_string_buffer(8 * 8 * 8 * 4))
    assert lib.vmapstep_mesh_count_valid(None, vol, 8, 8, 8, 0.0, vol, ws, nb.value, None) == -1
    assert lib.vmapstep_mesh_count_valid(vol, vol, 8, 8, 8, 0.0, None, ws, nb.value, None) == -1
    assert lib.vmapstep_mesh_count_valid(vol, vol, 8, 8, 1, 0.0, vol, ws, nb.value, None) == -2
    assert lib.vmapstep_mesh_count_valid(vol, vol, 8, 8, 8, 0.0, vol, ws + 4, nb.value, None) == -3
    assert lib.vmapstep_mesh_emit_valid(None, vol, 8, 8, 8, 0.0, None, vol, None, vol, None, 10, 10, ws, nb.value, None) == -1
    assert lib.vmapstep_mesh_emit_valid(vol, vol, 8, 8, 8, 0.0, None, None, None, vol, None, 10, 10, ws, nb.value, None) == -1
    assert lib.vmapstep_mesh_emit_valid(vol, vol, 8, 8, 8, 0.0, None, vol, None, vol, None, 10, 10, ws, nb.value - 1, None) == -3


def test_volume_refuses_bad_arguments_without_a_device():
    from vmap_amd import tsdf
    with pytest.raises(_lib.VmapStepError):
        tsdf.TSDFVolume((8, 8, 8), tc.grid_affine(), 0.1, device="cpu")
    with pytest.raises(_lib.VmapStepError):
        tsdf.TSDFVolume((8, 8, 8), tc.grid_affine(), 0.0, device="cuda:0")
    from vmap_amd.meshing import BoundingBox
    with pytest.raises(_lib.VmapStepError):
        tsdf.TSDFVolume.from_bound(BoundingBox(), trunc=0.1)
