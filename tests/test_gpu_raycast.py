"""GPU tier of the TSDF ray cast (vmap_amd/tsdf.py TSDFVolume.raycast; csrc/raycast_kernels.h).  Depth, status, normal, colour and the
brick classes are held bit for bit to the exact layer of the numpy checker (tests/raycast_oracle.py): every operation of the contract is
rounded on its own or is one fused operation, so there is no tolerance.  Nothing is held against an outside implementation.

Shapes (tests/raycast_cases.py): 19 x 26 x 33 (3 x 4 x 4 bricks, the last of every axis partial, with empty, free and mixed ones), 2 x 9 x 17
(one cell thick: one brick along i) and 5 x 9 x 70 (nz - 1 > 64: the brick kernel's lanes span two waves) under a rotated, anisotropic
affine; images 37 x 29 (no multiple of the 8 x 8 tile: partial tiles on both axes, a partial workgroup) and 64 x 48; three views, one an
unused slot, one from inside the volume; fused and noise-filled volumes."""
import numpy as np
import pytest
import torch

import icp_cases as ic
import icp_oracle as io
import raycast_cases as rcs
import raycast_oracle as ro
import tsdf_cases as tc
import tsdf_oracle as to
from conftest import AB_LIBRARY

pytestmark = pytest.mark.gpu
f32 = np.float32


def device_volume(shape, A, vol, trunc=rcs.TRUNC):
    from vmap_amd import tsdf
    v = tsdf.TSDFVolume(shape, A, trunc, color=vol["color"] is not None, device="cuda:0")
    v.tsdf.copy_(torch.from_numpy(np.asarray(vol["tsdf"], f32).reshape(shape)))
    v.weight.copy_(torch.from_numpy(np.asarray(vol["weight"], f32).reshape(shape)))
    if v.color is not None:
        v.color.copy_(torch.from_numpy(np.asarray(vol["color"], f32)))
    return v


def host(view):
    return dict(depth=view.depth.cpu().numpy(), status=view.status.cpu().numpy(), normal=None if view.normal is None else view.normal.cpu().numpy(),
                color=None if view.color is None else view.color.cpu().numpy())


@pytest.mark.parametrize("width,height", rcs.IMAGES)
@pytest.mark.parametrize("state", rcs.STATES)
@pytest.mark.parametrize("name", list(rcs.SHAPES))
def test_device_equals_the_exact_checker(name, state, width, height):
    vol, shape, A = rcs.volume(name, state)
    poses, intr = rcs.views_of(shape, A), ic.intrinsics_for(width, height)
    t32, M, N = ro.compose(A, poses)
    classes = ro.brick_classes(vol, shape, rcs.KW["min_weight"])
    want = ro.raycast(vol, shape, M, N, intr, width, height, exact=True, bricks=classes, color=True, **rcs.KW)
    v = device_volume(shape, A, vol)
    assert np.array_equal(v.brick_classes(rcs.KW["min_weight"]).cpu().numpy(), classes)
    view = v.raycast(poses, intr, width, height, **rcs.KW)
    got = host(view)
    assert rcs.same_bits(got, want) == []
    assert view.t_wc.dtype == np.float32 and np.array_equal(view.t_wc, t32)
    assert (got["status"][1] == ro.MISS).all() and (got["status"] == ro.HIT).any() == (want["status"] == ro.HIT).any()
    # without the classes: the same bits; the same call again: the same bits
    assert rcs.same_bits(host(v.raycast(poses, intr, width, height, use_bricks=False, **rcs.KW)), got) == []
    assert rcs.same_bits(host(v.raycast(poses, intr, width, height, **rcs.KW)), got) == []
    # one call over K views == K calls
    for k in range(len(poses)):
        one = host(v.raycast(poses[k], intr, width, height, **rcs.KW))
        assert rcs.same_bits(one, {key: got[key][k:k + 1] for key in got}) == [], k
    # the outputs that were not asked for are not made, and do not change the others
    bare = v.raycast(poses, intr, width, height, normals=False, color=False, **rcs.KW)
    assert bare.normal is None and bare.color is None and rcs.same_bits(host(bare), got, keys=("depth", "status")) == []


@pytest.mark.parametrize("name", list(rcs.SHAPES))
def test_class_table_in_global_memory_gives_the_same_bits(name):
    """The measurement build stages at most 16 bytes of class table in LDS: 19 x 26 x 33 (48 bricks) takes the global-memory path
    there, 5 x 9 x 70 (9) and 2 x 9 x 17 (2) the LDS path of that build; the product stages all three."""
    import re
    import os
    from conftest import ROOT
    with open(os.path.join(ROOT, "vmap_amd", "csrc", "launch_geometry.h")) as fh:
        ab_budget, budget = (int(x) for x in re.findall(r"kClassLdsBudget = (\d+);", fh.read()))
    vol, shape, A = rcs.volume(name, "fused")
    n_bricks = int(np.prod([ro.brick_dim(s) for s in shape]))
    assert n_bricks <= budget and (n_bricks > ab_budget) == (name == "19x26x33")
    poses, intr = rcs.views_of(shape, A), ic.intrinsics_for(37, 29)
    v = device_volume(shape, A, vol)
    got = host(v.raycast(poses, intr, 37, 29, **rcs.KW))
    assert rcs.same_bits(host(v.raycast(poses, intr, 37, 29, library=AB_LIBRARY, **rcs.KW)), got) == []
    assert np.array_equal(v.brick_classes(library=AB_LIBRARY).cpu().numpy(), v.brick_classes().cpu().numpy())
    assert (got["status"] != ro.MISS).any() and ((got["status"] == ro.HIT).any() or name == "2x9x17")   # the one-cell slab holds no crossing


def tracker(sc):
    from vmap_amd import odometry
    P = ic.PARAMS
    return odometry.DepthTracker(sc["intrinsics"], 64, 48, (10, 5, 4), dist_thresh=P.dist_thresh, cos_thresh=P.cos_thresh, band=P.band,
                                 min_depth=P.min_depth, max_depth=P.max_depth, damping=P.damping, pivot_rel=P.pivot_rel, eps=P.eps,
                                 min_inliers=P.min_inliers)


def test_track_to_volume_reproduces_the_cpu_path():
    """The tsdf_cases scene from icp_cases.offset(0.02, 1.0).  CPU path: the exact layer's raycast at the float32 rounding of the model
    pose, then icp_oracle.track.  Every stage is bit-exact against its checker, so the pose is the CPU path's bit for bit; its error
    falls below icp_cases.INITIAL_ERROR by raycast_cases.TRACK_FACTOR."""
    _, exact, shape, A = rcs.geometry_volumes()
    sc, P = ic.corner_scene(64, 48), ic.PARAMS
    t32, M, N = ro.compose(A, sc["t_wc_model"][None])
    model = ro.raycast(exact, shape, M, N, sc["intrinsics"], 64, 48, exact=True, normals=False,
                       **dict(rcs.GEOMETRY_KW, min_depth=P.min_depth, max_depth=P.max_depth))["depth"][0]
    t_model = t32[0].astype(np.float64)
    T0 = (ic.rigid_inverse(t_model) @ sc["t_wc_model"])[:3].reshape(12)
    want = io.track(sc["depth"], model, T0, sc["intrinsics"], ic.ITERATIONS, P)
    T_true = (ic.rigid_inverse(t_model) @ sc["t_wc_true"])[:3].reshape(12)
    cpu_factor = ic.INITIAL_ERROR / io.pose_error(want["pose"], T_true)
    trk = tracker(sc)
    trk.t_wc = sc["t_wc_model"].copy()
    res = trk.track_to_volume(device_volume(shape, A, exact, tc.TRUNC), sc["depth"])
    factor = ic.INITIAL_ERROR / io.pose_error(res.t_sm64[:3].reshape(12), T_true)
    print(f"the pose error falls by a factor {factor:.3f} on the device, {cpu_factor:.3f} on the CPU path")
    assert abs(cpu_factor - rcs.TRACK_FACTOR) <= 0.01 * rcs.TRACK_FACTOR
    assert res.ok and factor >= rcs.TRACK_FACTOR / 2
    assert np.array_equal(trk.t_wc_model, t_model)                                      # the float32 rounding is the model's pose
    assert np.array_equal(res.t_sm64[:3].reshape(12).view(np.uint64), np.asarray(want["pose"], np.float64).view(np.uint64))


def test_fuse_render_track_loop_over_four_frames():
    """Each round raycasts the volume at the last pose, tracks the next frame against it, then integrates that frame at the tracked
    pose: the loop the volume's view closes.  Frames 2 cm and 1 degree apart, the first integrated at its true pose."""
    from vmap_amd import tsdf
    sc = ic.corner_scene(64, 48)
    intr = sc["intrinsics"]
    poses = [ic.look_at(ic.EYE) @ ic.offset(0.02 * k, 1.0 * k) for k in range(4)]
    depth = [ic.render(T, intr, 64, 48) for T in poses]
    vol = tsdf.TSDFVolume((tc.GRID,) * 3, tc.grid_affine(), tc.TRUNC, device="cuda:0")
    vol.integrate(depth[0][None], poses[0][None], intr, max_depth=tc.MAX_DEPTH)
    trk = tracker(sc)
    trk.t_wc = poses[0].copy()
    for k in range(1, 4):
        res = trk.track_to_volume(vol, depth[k])
        assert res.ok, k
        assert np.abs(res.t_wc64 - poses[k]).max() < 5e-3, k                               # 1.9e-3 on the CPU path, every round
        vol.integrate(depth[k][None], res.t_wc64[None], intr, max_depth=tc.MAX_DEPTH)
    assert np.array_equal(trk.t_wc, res.t_wc64)


def test_volume_view_feeds_compare_depth_and_the_command_line(tmp_path, capsys):
    from vmap_amd import raster, tsdf
    _, exact, shape, A = rcs.geometry_volumes()
    sc = tc.scene()
    v = device_volume(shape, A, exact, tc.TRUNC)
    view = v.raycast(sc["t_wc"], sc["intrinsics"], tc.WIDTH, tc.HEIGHT, **rcs.GEOMETRY_KW)
    cmp_ = raster.compare_depth(view.depth, torch.from_numpy(sc["depth"]).cuda())          # VolumeView.depth, unchanged
    assert (cmp_["n_both"] > 0.6 * tc.WIDTH * tc.HEIGHT).all() and (cmp_["l1"] < tc.VOXEL / 2).all()
    assert view.color is None and view.normal.shape == (4, tc.WIDTH, tc.HEIGHT, 3)
    with pytest.raises(Exception):
        v.raycast(sc["t_wc"], sc["intrinsics"], tc.WIDTH, tc.HEIGHT, color=True, **rcs.GEOMETRY_KW)
    # python -m vmap_amd.tsdf ... --views OUT.npz, in process
    np.savez(tmp_path / "frames.npz", depth=sc["depth"], t_wc=sc["t_wc"], intrinsics=np.asarray(sc["intrinsics"]), rgb=sc["rgbx"][..., :3])
    out = str(tmp_path / "views.npz")
    assert tsdf.main([str(tmp_path / "frames.npz"), str(tmp_path / "scene.ply"), "--voxel-size", str(tc.VOXEL), "--trunc", str(tc.TRUNC),
                      "--max-depth", str(tc.MAX_DEPTH), "--views", out]) == 0
    assert "4 views" in capsys.readouterr().out
    with np.load(out) as f:
        assert f["depth"].shape == (4, tc.WIDTH, tc.HEIGHT) and f["status"].dtype == np.uint8 and f["normal"].shape[-1] == 3
        assert f["color"].shape == (4, tc.WIDTH, tc.HEIGHT, 4) and f["t_wc"].shape == (4, 4, 4)
        # The tool's volume is the exact box of the frames' points: the walls lie ON its faces, where nothing is behind them to cross.
        # The sphere is inside: the CPU checker on the same volume hits 96.6 % of the sphere's pixels, median error 0.18 voxel.
        hit, sphere = f["status"] == ro.HIT, sc["inst"] == tc.SPHERE_ID
        assert (hit & sphere).sum() > 0.9 * sphere.sum() and np.median(np.abs(f["depth"] - sc["depth"])[hit & sphere]) < tc.VOXEL / 2
        assert (f["color"][hit][:, 3] == 255).all()
