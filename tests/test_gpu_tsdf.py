"""GPU tier of TSDF fusion (vmap_amd/tsdf.py; csrc/tsdf_kernels.h) and of marching cubes over observed voxels (the valid mask of
csrc/mesh_kernels.h).  The volumes - tsdf, weight, colour - are held bit for bit to the exact layer of the numpy checker
(tests/tsdf_oracle.py): every operation of the contract is rounded on its own or is one fused operation, so there is no tolerance.
Meshes are held to the checker's masked marching cubes: faces and order exactly, coordinates and normals to the tolerances the unmasked
mesh tests use (tests/geom_checks.py: the kernel contracts a * b + c chains of the interpolation, the checker does not).

Shapes: 8 x 8 x 8 (less than a workgroup), 17 x 13 x 11 (n = 2431: partial waves, a partial workgroup, three workgroups), 5 x 9 x 70
(nz > 64: a wave wraps rows) under a rotated, anisotropic affine; images 64 x 48 and 37 x 29 with dirty depth; 1, 3, one more than the
kernel's LDS chunk, and 40 frames with shuffled, repeated slots and an unused slot among them."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import icp_cases as ic
import icp_oracle as io
import tsdf_cases as tc
import tsdf_oracle as to
from conftest import ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32

with open(os.path.join(ROOT, "vmap_amd", "csrc", "launch_geometry.h")) as _fh:
    CHUNK = int(re.search(r"kTsdfChunk = (\d+);", _fh.read()).group(1))

SHAPES = {"8x8x8": ((8, 8, 8), "grid"), "17x13x11": ((17, 13, 11), "grid"), "5x9x70": ((5, 9, 70), "oriented")}
KW = dict(trunc=0.2, margin=1, min_depth=0.1, max_depth=tc.MAX_DEPTH)


def affine_of(shape, kind):
    if kind == "oriented":
        return tc.oriented_affine()
    s = 1.5 / (max(shape) - 1)
    return np.array([[s, 0, 0, tc.LO], [0, s, 0, tc.LO], [0, 0, s, tc.LO]])


@functools.lru_cache(maxsize=None)
def frames(width, height, n):
    return tc.many_frames(width, height, n, seed=width + n)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def device_volume(shape, A, vol, trunc, max_weight):
    from vmap_amd import tsdf
    v = tsdf.TSDFVolume(shape, A, trunc, color=vol["color"] is not None, max_weight=max_weight, device="cuda:0")
    v.tsdf.copy_(torch.from_numpy(vol["tsdf"].reshape(shape)))
    v.weight.copy_(torch.from_numpy(vol["weight"].reshape(shape)))
    if v.color is not None:
        v.color.copy_(torch.from_numpy(vol["color"]))
    return v


def assert_same_volume(v, want):
    assert np.array_equal(bits(v.tsdf.cpu().numpy().reshape(-1)), bits(want["tsdf"]))
    assert np.array_equal(bits(v.weight.cpu().numpy().reshape(-1)), bits(want["weight"]))
    if want["color"] is not None:
        assert np.array_equal(bits(v.color.cpu().numpy()), bits(want["color"]))


def slots_of(n):
    if n < 40:
        return None                                                   # every slot in order, the unused slot 0 included
    return [int(s) for s in np.random.default_rng(n).integers(0, n, n + 7)]           # shuffled and repeated


@pytest.mark.parametrize("n_frames", [1, 3, CHUNK + 1, 40])
@pytest.mark.parametrize("width,height", [(64, 48), (37, 29)])
@pytest.mark.parametrize("name", list(SHAPES))
def test_volume_equals_the_exact_checker(name, width, height, n_frames):
    shape, kind = SHAPES[name]
    A = affine_of(shape, kind)
    sc = frames(width, height, max(n_frames, 2))                     # slot 0 is the unused one: K = 1 reads slot 1
    slots = [1] if n_frames == 1 else slots_of(n_frames)
    capped = False
    for color, obj_id, max_weight in ((False, None, 3.0), (True, None, 64.0), (False, tc.SPHERE_ID, 64.0), (True, tc.WALL_ID, 3.0)):
        start = to.empty(shape, color) if n_frames == 1 else tc.prefilled(shape, color, n_frames)
        want = to.integrate_f32(start, shape, A, sc["depth"], sc["t_wc"], sc["intrinsics"], rgbx=sc["rgbx"], inst=sc["inst"], obj_id=obj_id,
                                slots=slots, max_weight=max_weight, **KW)
        v = device_volume(shape, A, start, KW["trunc"], max_weight)
        v.integrate(sc["depth"], sc["t_wc"], sc["intrinsics"], rgb=sc["rgbx"] if color else None, inst=sc["inst"], obj_id=obj_id, slots=slots,
                    margin=KW["margin"], min_depth=KW["min_depth"], max_depth=KW["max_depth"])
        assert_same_volume(v, want)
        assert not np.array_equal(want["weight"], start["weight"])                       # the frames do reach the volume
        capped |= max_weight == 3.0 and bool((want["weight"] == 3).any())
    assert capped or n_frames == 1


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_call_equals_two_calls_over_its_halves(name):
    shape, kind = SHAPES[name]
    A, sc = affine_of(shape, kind), frames(64, 48, 40)
    slots = slots_of(40)
    out = []
    for parts in ([slots], [slots[:19], slots[19:]], [slots[:1], slots[1:CHUNK + 2], slots[CHUNK + 2:]]):
        v = device_volume(shape, A, tc.prefilled(shape, True, 9), KW["trunc"], 5.0)
        for part in parts:
            v.integrate(sc["depth"], sc["t_wc"], sc["intrinsics"], rgb=sc["rgbx"], slots=part, margin=1, min_depth=0.1, max_depth=tc.MAX_DEPTH)
        out.append([t.cpu().numpy().tobytes() for t in (v.tsdf, v.weight, v.color)])
    assert out[0] == out[1] == out[2]


def test_frames_that_see_nothing_leave_every_bit():
    """A volume wholly outside every frustum (behind the cameras), and a batch of all-zero poses over a volume in view."""
    shape = (17, 13, 11)
    sc = frames(64, 48, 5)
    start = tc.prefilled(shape, True, 4)
    start["tsdf"][:7] = [np.nan, np.inf, -np.inf, -0.0, 1e-42, 3.0, -7.0]          # bits a rewrite or a no-op update would not keep
    behind = np.array([[0.05, 0, 0, 5.0], [0, 0.05, 0, 5.0], [0, 0, 0.05, 5.0]])
    zero = dict(sc, t_wc=np.zeros_like(sc["t_wc"]))
    for A, frames_ in ((behind, sc), (affine_of(shape, "grid"), zero)):
        v = device_volume(shape, A, start, 0.2, 64.0)
        v.integrate(frames_["depth"], frames_["t_wc"], sc["intrinsics"], rgb=sc["rgbx"], max_depth=tc.MAX_DEPTH)
        assert_same_volume(v, start)
        assert_same_volume(v, to.integrate_f32(start, shape, A, frames_["depth"], frames_["t_wc"], sc["intrinsics"], rgbx=sc["rgbx"], trunc=0.2,
                                               max_depth=tc.MAX_DEPTH))


@pytest.mark.parametrize("name", list(SHAPES))
def test_voxel_centres_are_grid_points(name):
    """The centres the exact layer integrates at - which the kernel's volumes equal bit for bit - are meshing.grid_points'."""
    from vmap_amd import meshing
    shape, kind = SHAPES[name]
    A = affine_of(shape, kind)
    assert np.array_equal(bits(meshing.grid_points(shape, A).cpu().numpy()), bits(to.centers_f32(shape, A)))


# ---- marching cubes over valid points --------------------------------------------------------------------------------------------------
def assert_mesh_equals_checker(vol, valid, mesh, edges, affine, level=0.0):
    v, f, n, e, _ = to.marching_cubes(vol, valid, level, affine)
    gv, gf, gn, _ = mesh.numpy()
    assert np.array_equal(gf, f) and np.array_equal(edges.cpu().numpy(), e.astype(np.int32))
    assert gv.shape == v.shape and np.abs(gv - v).max() < 1e-5 * (np.abs(v).max() + 1)
    g = to.masked_gradient(vol, valid).reshape(-1, 3)
    stride = np.array([vol.shape[1] * vol.shape[2], vol.shape[2], 1])
    ok = (np.linalg.norm(g[e // 3], axis=1) > 1e-6) | (np.linalg.norm(g[e // 3 + stride[e % 3]], axis=1) > 1e-6)
    ok &= np.linalg.norm(n, axis=1) > 0.5
    assert np.abs(gn[ok] - n[ok]).max() < 1e-4
    assert np.isfinite(gv).all() and np.isfinite(gn).all() and len(np.unique(gf)) == len(gv)      # no vertex is unreferenced


@pytest.mark.parametrize("seed", range(6))
def test_masked_mesh_equals_the_checker_on_random_volumes(seed):
    from vmap_amd import meshing
    rng = np.random.default_rng(seed)
    vol = rng.uniform(-1, 1, (9, 7, 5)).astype(f32)
    A = tc.oriented_affine() if seed % 2 else None
    t = torch.from_numpy(vol).cuda()
    plain = meshing.extract_mesh(t, 0.0, A)
    ones, ones_edges = meshing.extract_mesh(t, 0.0, A, valid=torch.ones(vol.shape, dtype=torch.uint8, device="cuda"), return_edges=True)
    for a, b in zip(plain.numpy()[:3], ones.numpy()[:3]):
        assert a.tobytes() == b.tobytes()                                                         # all ones: the unmasked mesh bit for bit
    assert meshing.extract_mesh(t, 0.0, A, valid=np.zeros(vol.shape, bool)) is None
    assert meshing.extract_mesh(t, 0.0, A, valid=np.zeros(vol.shape, bool), return_edges=True) == (None, None)
    valid = rng.uniform(size=vol.shape) < (0.95, 0.8, 0.6)[seed % 3]
    poisoned = np.where(valid, vol, np.nan).astype(f32)                                           # an invalid value must never be used
    mesh, edges = meshing.extract_mesh(torch.from_numpy(poisoned).cuda(), 0.0, A, valid=valid, return_edges=True)
    assert_mesh_equals_checker(poisoned, valid, mesh, edges, A)


@pytest.fixture(scope="module")
def fused():
    """The 32^3 geometry scene fused on the device with colour, and the exact layer's volume."""
    from vmap_amd import tsdf
    sc, shape, A = tc.scene(), (tc.GRID,) * 3, tc.grid_affine()
    v = tsdf.TSDFVolume(shape, A, tc.TRUNC, color=True, device="cuda:0")
    v.integrate(sc["depth"], sc["t_wc"], sc["intrinsics"], rgb=sc["rgbx"], max_depth=tc.MAX_DEPTH)
    want = to.integrate_f32(to.empty(shape, True), shape, A, sc["depth"], sc["t_wc"], sc["intrinsics"], rgbx=sc["rgbx"], trunc=tc.TRUNC,
                            max_depth=tc.MAX_DEPTH)
    return dict(volume=v, want=want, shape=shape, A=A, checker=to.extract(want, shape, A))


def test_fused_mesh_equals_the_checker(fused):
    from vmap_amd import meshing
    v, want, shape = fused["volume"], fused["want"], fused["shape"]
    assert_same_volume(v, want)
    mesh = v.extract_mesh()
    pos, faces, nrm, edges, t = fused["checker"]
    assert len(pos) >= tc.MIN_VERTICES
    valid = want["weight"].reshape(shape) >= 1
    _, dev_edges = meshing.extract_mesh(torch.neg(v.tsdf), 0.0, fused["A"], valid=v.weight >= 1, return_edges=True)
    assert_mesh_equals_checker(-want["tsdf"].reshape(shape), valid, mesh, dev_edges, fused["A"])
    # geometry, normals and winding: the issue's caps on the device's own mesh
    gv, gf, gn, gc = mesh.numpy()
    d = np.abs(tc.true_sdf(gv)) / tc.VOXEL
    assert (d > 0.5).mean() <= tc.MAX_SHARE_BEYOND_HALF and d.max() <= tc.MAX_WORST_VOXELS
    out = tc.excluded(gv)
    assert out.mean() < tc.MAX_EXCLUDED_SHARE and ((gn * tc.outward(gv)).sum(1)[~out] > 0).all()
    fn = np.cross(gv[gf[:, 1]] - gv[gf[:, 0]], gv[gf[:, 2]] - gv[gf[:, 0]]).astype(np.float64)
    assert ((fn[:, None, :] * gn[gf]).sum(-1)[~out[gf].any(1)] > 0).all()
    # colours: the lerp in float32 may land on the other side of a rounding tie than the checker's: one level
    assert gc.dtype == np.uint8 and gc.shape == gv.shape
    assert np.abs(gc.astype(np.int32) - to.vertex_colors(want, shape, edges, t).astype(np.int32)).max() <= 1
    # the component options go through keep_components: the largest component alone is a sub-mesh
    big = v.extract_mesh(largest_components=1)
    assert 0 < len(big.faces) <= len(gf) and big.vertex_colors is not None
    assert v.extract_mesh(min_weight=1e9) is None
    v2 = type(v)(shape, fused["A"], tc.TRUNC, device="cuda:0")
    assert v2.extract_mesh() is None                                                              # an empty volume: no surface
    v2.integrate(tc.scene()["depth"], tc.scene()["t_wc"], tc.scene()["intrinsics"], max_depth=tc.MAX_DEPTH)
    assert v2.extract_mesh().vertex_colors is None and np.array_equal(v2.extract_mesh().numpy()[1], gf)
    v2.reset()
    assert not v2.tsdf.any() and not v2.weight.any() and v2.extract_mesh() is None


# Composition.  Accuracy and completion of the device's mesh against those of the checker's mesh through the same calc_3d_metric call,
# measured on the device at N = 20000: accuracy 1.059257e-02 against 1.059289e-02 (a difference of 3.2e-7 m), completion 2.801089e-02
# against 2.801089e-02 (none in seven digits) - the two meshes have the same faces and coordinates within 1e-5 relative, and the samples
# are drawn from the same Philox streams.  The margin is twice the larger measured difference.
METRIC_MARGIN = 6.4e-7


def test_fused_mesh_through_calc_3d_metric(fused):
    from vmap_amd import evaluation, meshing
    gt_v, gt_f = ic.corner_mesh()
    box = meshing.BoundingBox(center=[(tc.LO + tc.HI) / 2] * 3, R=np.eye(3), extent=[tc.HI - tc.LO] * 3)
    gt = evaluation.crop_to_box(meshing.Mesh(torch.from_numpy(gt_v).cuda(), torch.from_numpy(gt_f).cuda(), None), box)
    pos, faces, nrm, _, _ = fused["checker"]
    checker = meshing.Mesh(torch.from_numpy(pos).cuda(), torch.from_numpy(faces).cuda(), torch.from_numpy(nrm).cuda())
    got = evaluation.calc_3d_metric(fused["volume"].extract_mesh(), gt, N=20000, box=box)
    want = evaluation.calc_3d_metric(checker, gt, N=20000, box=box)
    print(f"accuracy {got[0][0]:.9e} / {want[0][0]:.9e}, completion {got[1][0]:.9e} / {want[1][0]:.9e}, ratios {got[2:]} / {want[2:]}")
    assert abs(got[0][0] - want[0][0]) <= METRIC_MARGIN and abs(got[1][0] - want[1][0]) <= METRIC_MARGIN
    assert got[0][0] < tc.VOXEL / 2                                     # the surface lies within half a voxel of the GT on average


def test_tracker_converges_on_the_fused_mesh(fused):
    from vmap_amd import odometry
    P = ic.PARAMS
    sc = ic.corner_scene(64, 48)
    trk = odometry.DepthTracker(sc["intrinsics"], 64, 48, (10, 5, 4), dist_thresh=P.dist_thresh, cos_thresh=P.cos_thresh, band=P.band,
                                min_depth=P.min_depth, max_depth=P.max_depth, damping=P.damping, pivot_rel=P.pivot_rel, eps=P.eps,
                                min_inliers=P.min_inliers)
    trk.t_wc = sc["t_wc_model"].copy()
    res = trk.track_to_mesh(fused["volume"].extract_mesh(), sc["depth"])
    err = io.pose_error((ic.rigid_inverse(sc["t_wc_model"]) @ res.t_wc64)[:3].reshape(12), sc["T_true"])
    print(f"pose error {err:.6e}: a factor {ic.INITIAL_ERROR / err:.2f} below the initial {ic.INITIAL_ERROR:.6e}")
    assert res.ok and err * tc.TRACK_FACTOR / 2 <= ic.INITIAL_ERROR


def test_fuse_object_on_a_two_object_store():
    from vmap_amd import keyframes, tsdf
    sc = tc.scene()
    store = keyframes.FrameStore(6, tc.WIDTH, tc.HEIGHT, device="cuda:0")
    slots = [store.put(torch.from_numpy(sc["rgbx"][k, :, :, :3].copy()), torch.from_numpy(sc["depth"][k]), torch.from_numpy(sc["inst"][k]),
                       torch.from_numpy(sc["t_wc"][k]), k) for k in range(len(sc["depth"]))]
    box2d = (0, tc.WIDTH - 1, 0, tc.HEIGHT - 1)
    objects = {}
    for oid in (tc.SPHERE_ID, tc.WALL_ID):
        objects[oid] = keyframes.ObjectKeyframes(store, oid, slots[0], box2d)
        for s in slots[1:]:
            objects[oid].append(s, box2d)
    mesh = tsdf.fuse_object(objects[tc.SPHERE_ID], sc["intrinsics"], tc.VOXEL, tc.TRUNC, color=True, max_depth=tc.MAX_DEPTH)
    v, f, n, c = mesh.numpy()
    assert len(v) > 200 and c is not None and len(np.unique(f)) == len(v)
    assert (np.abs(np.linalg.norm(v - ic.SPHERE_CENTER, axis=1) - ic.SPHERE_RADIUS) <= 1.5 * tc.VOXEL).all()
    assert (v.min(1) > 1.5 * tc.VOXEL).all()                                                      # none on the walls
    walls = tsdf.fuse_object(objects[tc.WALL_ID], sc["intrinsics"], tc.VOXEL, tc.TRUNC, max_depth=tc.MAX_DEPTH)
    assert len(walls.vertices) > len(v) and walls.vertex_colors is None


def test_command_line_writes_the_mesh_of_a_frames_file(tmp_path, capsys):
    """python -m vmap_amd.tsdf FRAMES.npz OUT.ply, in process: the evaluation tool's frames file plus rgb and inst."""
    from vmap_amd import meshing, tsdf
    sc = tc.scene()
    np.savez(tmp_path / "frames.npz", depth=sc["depth"], t_wc=sc["t_wc"], intrinsics=np.asarray(sc["intrinsics"]), rgb=sc["rgbx"][..., :3],
             inst=sc["inst"])
    out = str(tmp_path / "sphere.ply")
    args = [str(tmp_path / "frames.npz"), out, "--voxel-size", str(tc.VOXEL), "--trunc", str(tc.TRUNC), "--max-depth", str(tc.MAX_DEPTH)]
    assert tsdf.main(args + ["--obj-id", str(tc.SPHERE_ID)]) == 0
    said = capsys.readouterr().out
    v = meshing.load_mesh(out).numpy()[0]
    assert f"{len(v)} vertices" in said and len(v) > 200
    assert (np.abs(np.linalg.norm(v - ic.SPHERE_CENTER, axis=1) - ic.SPHERE_RADIUS) <= 1.5 * tc.VOXEL).all()
