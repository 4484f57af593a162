"""GPU tier of the depth tracker (vmap_amd/odometry.py; csrc/icp_kernels.h): every case is held bit for bit to the exact layer of the
numpy checker (tests/icp_oracle.py) - the maps of every level, the 29 integer sums, the log, and the float64 pose after every
iteration.  Integer sums and a rational rotation have no tolerance.  Sizes: 64 x 48 and 37 x 29 with three levels (odd sizes halve by
ceil and clamp their 2 x 2 blocks), 8 x 8 (less than a wave), 70 x 50 (several waves, a partial one, 14 workgroups - and 2 or 3
through ``grid_cap``, so that a lane accumulates several pixels)."""
import numpy as np
import pytest
import torch

import icp_cases as ic
import icp_oracle as io

pytestmark = pytest.mark.gpu
P = ic.PARAMS
CFG = dict(dist_thresh=P.dist_thresh, cos_thresh=P.cos_thresh, band=P.band, min_depth=P.min_depth, max_depth=P.max_depth, damping=P.damping,
           pivot_rel=P.pivot_rel, eps=P.eps, min_inliers=P.min_inliers)


def params(**kw):
    return io.Params(**dict(P.__dict__, **kw)), dict(CFG, **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(a.view(view), b.view(view))


def dirty(depth, seed=3):
    """NaN, inf, -inf, 0, a negative value, values outside (min_depth, max_depth] and a hole, on top of the sphere's silhouette - a
    depth edge inside 2 x 2 blocks and across central differences at every level."""
    d = depth.copy()
    rng = np.random.default_rng(seed)
    W, H = d.shape
    for v in (np.nan, np.inf, -np.inf, 0.0, 0.0, -1.0, 0.05, 11.0):
        d[rng.integers(W), rng.integers(H)] = v
    d[W // 2:W // 2 + 3, H // 3:H // 3 + 2] = 0.0
    return d


def run_case(depth, model_depth, sc, coarse_first, p, kw, grid_cap=0, t_init=None):
    """track_depth against the checker: maps, the sums of one iteration at every level, log, sums and pose of every iteration."""
    from vmap_amd import odometry
    intr = sc["intrinsics"]
    by_level = tuple(reversed(coarse_first))
    levels = len(by_level)
    t_model = sc["t_wc_model"]
    t_init = t_model if t_init is None else t_init
    T0 = (ic.rigid_inverse(t_model) @ t_init)[:3].reshape(12)
    want_src, want_mod = io.maps(depth, intr, levels, p), io.maps(model_depth, intr, levels, p)
    want = io.track_maps(want_src, want_mod, T0, intr, by_level, p)
    mk = dict(min_depth=p.min_depth, max_depth=p.max_depth, band=p.band)
    src, mod = odometry.depth_maps(depth, intr, levels, **mk), odometry.depth_maps(model_depth, intr, levels, **mk)
    for level in range(levels):
        assert same_bits(src.entries[level].cpu().numpy(), want_src[level]), ("source map", level)
        assert same_bits(mod.entries[level].cpu().numpy(), want_mod[level]), ("model map", level)
        assert np.array_equal(src.has_normal[level].cpu().numpy(), (want_src[level][..., :3] != 0).any(-1))
        got = odometry.icp_sums(src, mod, level, T0, dist_thresh=p.dist_thresh, cos_thresh=p.cos_thresh, grid_cap=grid_cap).cpu().numpy()
        assert np.array_equal(got, io.sums(want_src[level], want_mod[level], io.level_camera(intr, level), T0, p)), ("sums", level)
    res = odometry.track_depth(depth, model_depth, t_model, t_init, intr, iterations=coarse_first, grid_cap=grid_cap, **kw)
    assert np.array_equal(res.sums, want["sums"])
    assert same_bits(res.log, want["log"])
    assert same_bits(res.poses, want["poses"])
    assert same_bits(res.t_sm64[:3].reshape(12), want["pose"])
    ok, fraction = io.summary(want, by_level[0], depth.shape[0] * depth.shape[1])
    assert res.ok == ok and res.inlier_fraction == fraction
    T = np.eye(4)
    T[:3] = want["pose"].reshape(3, 4)
    assert same_bits(res.t_wc64, t_model @ T)                                          # the documented pose: t_wc_model @ T
    assert res.t_wc.dtype == torch.float32 and res.t_wc.is_cuda and same_bits(res.t_wc.cpu().numpy(), (t_model @ T).astype(np.float32))
    return res, want


def test_corner_scene_converges_to_the_checkers_pose():
    """64 x 48, three levels, (10, 5, 4) iterations from 2 cm and 1 degree: the device pose is the exact checker's bit for bit, and
    that pose is within twice the recorded ratio of the plain float64 layer's error against the true pose (tests/icp_cases.py)."""
    sc = ic.corner_scene(64, 48)
    res, want = run_case(sc["depth"], sc["model_depth"], sc, (10, 5, 4), P, CFG)
    plain = io.track_plain(sc["depth"], sc["model_depth"], sc["T_init"], sc["intrinsics"], ic.ITERATIONS, P)
    e0, e_plain = io.pose_error(sc["T_init"], sc["T_true"]), io.pose_error(plain, sc["T_true"])
    e_dev = io.pose_error(res.t_sm64[:3].reshape(12), sc["T_true"])
    print(f"initial {e0:.6e} plain {e_plain:.6e} device {e_dev:.6e}")
    assert e_plain * 10 <= e0 and e_dev <= 2 * ic.EXACT_OVER_PLAIN * e_plain
    assert res.ok and res.inlier_fraction > 0.5
    assert np.abs(res.t_wc64 - sc["t_wc_true"]).max() < 2e-3


@pytest.mark.parametrize("width,height,coarse_first,grid_cap", [
    (37, 29, (4, 3, 3), 0), (8, 8, (3,), 0), (70, 50, (3,), 0), (70, 50, (2, 3), 2), (70, 50, (3,), 3)],
    ids=["37x29", "8x8", "70x50", "70x50_grid2", "70x50_grid3"])
def test_sizes_equal_the_exact_checker(width, height, coarse_first, grid_cap):
    """Odd sizes with ceil-halving and clamped blocks at every level; less than a wave; several waves with a partial one over 14
    workgroups, and over 2 or 3 with every lane taking several pixels.  Dirty depths (NaN, inf, 0, out of range) and the silhouette's
    depth edges are in every case."""
    sc = ic.corner_scene(width, height, sphere=width > 8)                            # 8 x 8: the bare corner, or too few pixels have normals
    res, want = run_case(dirty(sc["depth"]) if width > 8 else sc["depth"], sc["model_depth"], sc, coarse_first, P, CFG, grid_cap=grid_cap)
    assert res.ok and (want["log"][:, 0] >= P.min_inliers).all() and (want["log"][:, 2] != io.DEGENERATE).all()


def test_a_frame_without_a_valid_pixel():
    """Every iteration is DEGENERATE, the pose is the initial one, ok is false."""
    sc = ic.corner_scene(37, 29)
    empty = np.full((37, 29), np.nan, np.float32)
    empty[::2] = 0.0
    t_init = sc["t_wc_model"] @ ic.offset(0.01, 0.5)
    res, want = run_case(empty, sc["model_depth"], sc, (2, 2, 2), P, CFG, t_init=t_init)
    assert (res.log[:, 2] == io.DEGENERATE).all() and (res.log[:, [0, 1, 3]] == 0).all() and not res.ok and res.inlier_fraction == 0.0
    T0 = (ic.rigid_inverse(sc["t_wc_model"]) @ t_init)[:3].reshape(12)
    assert same_bits(res.poses, np.tile(T0, (6, 1))) and same_bits(res.t_sm64[:3].reshape(12), T0)


def test_a_single_plane_is_degenerate_without_a_nan():
    """Rank-deficient normal equations: the pivot test fires in every iteration, nothing is NaN, the pose does not move."""
    sc = ic.corner_scene(64, 48, sphere=False, planes=(2,))
    res, want = run_case(sc["depth"], sc["model_depth"], sc, (2, 2), P, CFG)
    assert (res.log[:, 2] == io.DEGENERATE).all() and (res.log[:, 0] > 100).all() and not res.ok
    assert np.isfinite(res.log).all() and np.isfinite(res.poses).all() and np.isfinite(res.t_wc64).all()
    assert same_bits(res.poses[-1], res.poses[0])


def test_the_early_finish_flag_skips_the_rest_of_a_level():
    """eps = 1e-3: the coarse level's second iteration ends with |x|^2 < eps^2; its other eight rows are SKIPPED, with zero sums and
    the unchanged pose, and the next level starts with the flag lowered."""
    p, kw = params(eps=1e-3)
    sc = ic.corner_scene(64, 48)
    res, want = run_case(sc["depth"], sc["model_depth"], sc, (10, 5, 4), p, kw)
    status = res.log[:, 2]
    assert status[:2].tolist() == [io.OK, io.OK] and res.log[0, 3] >= 1e-6 > res.log[1, 3]
    assert (status[2:10] == io.SKIPPED).all() and (res.sums[2:10] == 0).all() and same_bits(res.poses[2:10], np.tile(res.poses[1], (8, 1)))
    assert status[10] == io.OK and res.sums[10, 0] > 0 and res.ok


def test_two_fresh_trackers_agree_byte_for_byte_and_the_pose_advances():
    from vmap_amd import odometry
    sc = ic.corner_scene(64, 48)
    out = []
    for _ in range(2):
        trk = odometry.DepthTracker(sc["intrinsics"], 64, 48, (10, 5, 4), **CFG)
        trk.set_model(sc["model_depth"], sc["t_wc_model"])
        a = trk.track(sc["depth"])
        assert a.ok and same_bits(trk.t_wc, a.t_wc64)                                 # on ok the last pose advances ...
        b = trk.track(sc["depth"])                                                    # ... and is the next call's first guess
        out.append((a, b))
    for x, y in zip(out[0], out[1]):
        assert x.sums.tobytes() == y.sums.tobytes() and x.log.tobytes() == y.log.tobytes() and x.poses.tobytes() == y.poses.tobytes()
        assert x.t_wc64.tobytes() == y.t_wc64.tobytes() and torch.equal(x.t_wc, y.t_wc)
    want = io.track(sc["depth"], sc["model_depth"], (ic.rigid_inverse(sc["t_wc_model"]) @ out[0][0].t_wc64)[:3].reshape(12), sc["intrinsics"],
                    ic.ITERATIONS, P)
    assert same_bits(out[0][1].poses, want["poses"])


def test_bad_arguments_leave_the_state_untouched():
    from vmap_amd import _lib, odometry
    sc = ic.corner_scene(64, 48)
    trk = odometry.DepthTracker(sc["intrinsics"], 64, 48, (10, 5, 4), **CFG)
    with pytest.raises(_lib.VmapStepError):
        trk.track(sc["depth"])                                                        # no model yet
    trk.set_model(sc["model_depth"], sc["t_wc_model"])
    model_before, pose_before = trk._model.clone(), trk.t_wc.copy()
    bad_pose = sc["t_wc_model"].copy()
    bad_pose[0, 3] = np.nan
    for call in (lambda: trk.track(sc["depth"][:, :40]), lambda: trk.track(sc["depth"], t_wc_init=bad_pose),
                 lambda: trk.set_model(sc["model_depth"].T, sc["t_wc_model"]), lambda: trk.set_model(sc["model_depth"], bad_pose),
                 lambda: odometry.track_depth(sc["depth"], sc["model_depth"], sc["t_wc_model"], sc["t_wc_model"], sc["intrinsics"], iterations=(10, 0, 4), **CFG),
                 lambda: odometry.track_depth(sc["depth"], sc["model_depth"][:32], sc["t_wc_model"], sc["t_wc_model"], sc["intrinsics"], **CFG)):
        with pytest.raises(_lib.VmapStepError):
            call()
    assert torch.equal(trk._model, model_before) and same_bits(trk.t_wc, pose_before)
    fresh = odometry.DepthTracker(sc["intrinsics"], 64, 48, (10, 5, 4), **CFG)
    fresh.set_model(sc["model_depth"], sc["t_wc_model"])
    assert trk.track(sc["depth"]).poses.tobytes() == fresh.track(sc["depth"]).poses.tobytes()


def test_track_to_mesh_on_the_scenes_own_mesh():
    """The scene as a mesh of small triangles, rasterised at the last pose by raster.rasterize, is the model; the frame is ray-cast
    from the true pose.  The tracker returns ok and lands near the true pose (the mesh is a polyhedral sphere: 5 mm)."""
    from vmap_amd import odometry
    sc = ic.corner_scene(64, 48)
    trk = odometry.DepthTracker(sc["intrinsics"], 64, 48, (10, 5, 4), **CFG)
    trk.t_wc = sc["t_wc_model"].copy()
    res = trk.track_to_mesh(ic.corner_mesh(), sc["depth"])
    assert res.ok and res.inlier_fraction > 0.5
    before = np.abs(sc["t_wc_model"] - sc["t_wc_true"]).max()
    assert np.abs(res.t_wc64 - sc["t_wc_true"]).max() < min(5e-3, before / 3)
    assert same_bits(trk.t_wc, res.t_wc64)
