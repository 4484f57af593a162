"""Object bounds, GPU tier: vmapstep_unproject_count / _emit against the float64 checker on a synthetic keyframe scene,
vmapstep_obb_extents against the checker and against itself under other launch geometries, get_bounds end to end (batch against
single calls, containment, extents and volume against the true boxes), the returned box through Trainer.meshing and
calc_3d_metric, and one case at Replica frame size.

Rounding bounds, derived from the kernels' operation order (csrc/bounds_kernels.h):
- unprojection: xc = ((w - cx) / fx) * d carries 2.5 roundings (w - cx is exact here or one more), each row is three nested fmas, so a
  coordinate is off by at most 2.5 ulp of the x / y terms + 3 ulp of the partial sums <= 6 * 2^-24 * (sum_j |T_ij pc_j| + |t_i|);
- extents: one product and two fmas: 3 * 2^-24 * sum_i |q_i r_i| <= the issue's 2^-22 * sum_i |q_i r_i| at the extreme point."""
import math

import numpy as np
import pytest
import torch

import bounds_oracle as bo
from test_bounds import THETA, scene_conditions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _mods():
    from vmap_amd import bounds, keyframes
    return bounds, keyframes


def _store_scene(scene, extra_ids=()):
    """The scene in a FrameStore, one ObjectKeyframes per box (+ one per extra id: objects no pixel shows), every frame a keyframe."""
    _, kf = _mods()
    store = kf.FrameStore(len(scene.frames), scene.W, scene.H, device=DEV)
    slots = []
    for i, f in enumerate(scene.frames):
        rgb = torch.zeros(scene.W, scene.H, 3, dtype=torch.uint8)
        slots.append(store.put(rgb, torch.from_numpy(f["depth"]), torch.from_numpy(f["inst"]), torch.from_numpy(f["t_wc"]), i))
    objs = []
    for oid in [b["id"] for b in scene.boxes] + list(extra_ids):
        ok = kf.ObjectKeyframes(store, oid, slots[0], (0, 0, scene.W, scene.H), keyframe_buffer_size=len(slots))
        for s in slots[1:]:
            ok.append(s, (0, 0, scene.W, scene.H))
        objs.append(ok)
    return store, objs


@pytest.fixture(scope="module")
def scene():
    return bo.Scene()


def test_object_points_match_the_checker(scene):
    bounds, _ = _mods()
    _, objs = _store_scene(scene, extra_ids=(11,))
    pts, off = bounds.object_points(objs, scene.k4)
    pts = pts.cpu().numpy()
    assert off[0] == 0 and off[-1] == len(pts) and off[3] == off[2]                  # id 11: an empty segment
    total_candidates = 0
    for o, b in enumerate(scene.boxes):
        ref, scale = scene.cloud(b["id"])
        got = pts[off[o]:off[o + 1]]
        assert len(got) == len(ref) > 1000
        err = np.abs(got.astype(np.float64) - ref)
        bound = 6 * 2.0 ** -24 * scale
        print(f"id {b['id']}: {len(ref)} points, worst error / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound)
        total_candidates += sum(int(((f["inst"] == b["id"]) | (f["inst"] == -1)).sum()) for f in scene.frames)
    assert len(pts) < total_candidates                                             # unknown ids and zero depths are absent
    # repeat: bit-identical; a sub-list gives the same segments
    pts2, off2 = bounds.object_points(objs, scene.k4)
    assert np.array_equal(off, off2) and np.array_equal(pts, pts2.cpu().numpy())
    p1, o1 = bounds.object_points(objs[1:2], scene.k4)
    assert np.array_equal(p1.cpu().numpy(), pts[off[1]:off[2]])
    boxes = bounds.get_bounds(objs, scene.k4)
    assert boxes[2] is None and boxes[0] is not None and boxes[1] is not None
    assert objs[2].get_bound(scene.k4) is None


@pytest.mark.parametrize("n_objects", [1, 2])
def test_object_points_match_the_checker_past_one_scan_chunk(n_objects):
    """Two keyframes of 1200 x 680 are 797 blocks each: one object has 1594 block totals, two have 3188, so unproject_scan leaves its
    first chunk of 1024 inside an object (and between objects).  Point by point against the checker, with the small scene's bound."""
    bounds, _ = _mods()
    big = bo.Scene(width=1200, height=680, fx=1000.0, n_views=2, radius=3.0, seed=2)
    _, objs = _store_scene(big)
    pts, off = bounds.object_points(objs[:n_objects], big.k4)
    pts = pts.cpu().numpy()
    assert off[0] == 0 and off[-1] == len(pts) and len(off) == n_objects + 1
    for o, b in enumerate(big.boxes[:n_objects]):
        ref, scale = big.cloud(b["id"])
        got = pts[off[o]:off[o + 1]]
        assert len(got) == len(ref) > 100_000
        err = np.abs(got.astype(np.float64) - ref)
        bound = 6 * 2.0 ** -24 * scale
        print(f"id {b['id']}: {len(ref)} points, worst error / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound)


def _clouds(rng, sizes):
    parts = [(rng.standard_normal((n, 3)) * rng.uniform(0.05, 30.0) * (1.0, 2.0, 0.3) + rng.uniform(-3, 3, 3)).astype(np.float32) for n in sizes]
    return parts, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("K", [100, 1100])
@pytest.mark.parametrize("shared", [True, False])
def test_obb_extents_match_the_checker_and_do_not_depend_on_the_geometry(K, shared):
    bounds, _ = _mods()
    rng = np.random.default_rng(K + shared)
    sizes = [0, 1, 5, 70001, 700]
    parts, off = _clouds(rng, sizes)
    pts = torch.from_numpy(np.concatenate(parts)).to(DEV)
    rot = bo.random_rotations(rng, K if shared else K * len(sizes)).astype(np.float32)
    rot = rot if shared else rot.reshape(len(sizes), K, 3, 3)
    centre = np.stack([p.mean(0) if len(p) else np.zeros(3) for p in parts]).astype(np.float32)
    for c in (None, centre):
        lo, hi = bounds.extents(pts, rot, off, center=c)
        lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
        assert np.all(lo_h[0] == np.inf) and np.all(hi_h[0] == -np.inf)            # no points: (+inf, -inf)
        for o in range(1, len(sizes)):
            r = rot if shared else rot[o]
            lo64, hi64, slo, shi = bo.extents64(parts[o], r, None if c is None else c[o])
            elo, ehi = np.abs(lo_h[o] - lo64), np.abs(hi_h[o] - hi64)
            assert np.all(elo <= 2.0 ** -22 * slo) and np.all(ehi <= 2.0 ** -22 * shi), (o, (elo / slo).max() * 2 ** 22, (ehi / shi).max() * 2 ** 22)
        # the same call again, and the points spread over other numbers of workgroups: bit-identical
        for chunks in (0, 1, 7, 40, 137):
            lo2, hi2 = bounds.extents(pts, rot, off, center=c, point_chunks=chunks)
            assert torch.equal(lo.view(torch.int32), lo2.view(torch.int32)) and torch.equal(hi.view(torch.int32), hi2.view(torch.int32)), chunks


def test_get_bounds_end_to_end(scene):
    bounds, _ = _mods()
    _, objs = _store_scene(scene)
    boxes = bounds.get_bounds(objs, scene.k4)
    pts, off = bounds.object_points(objs, scene.k4)
    clouds = [pts[off[o]:off[o + 1]].cpu().numpy() for o in range(len(objs))]
    assert sum(len(c) for c in clouds) > 20000
    msgs = scene_conditions(scene, boxes, clouds, "hip")
    for o, ok in enumerate(objs):                                  # one call for all objects = the per-object calls, bit for bit
        single = ok.get_bound(scene.k4)
        for k in ("center", "R", "extent"):
            np.testing.assert_array_equal(getattr(single, k), getattr(boxes[o], k))
    # the numpy backend on the same float32 clouds: it may pick another box among near-ties; it meets the same conditions
    host = bounds.oriented_bounds(np.concatenate(clouds), off, backend="numpy")
    msgs += scene_conditions(scene, host, clouds, "numpy on the device's cloud")
    print("\n".join(msgs))
    # and the search driven directly: volumes never above the coarse set's best
    _, info = bounds.oriented_bounds(pts, off, return_info=True)
    assert np.all(info["volume"] <= info["coarse_volume"]), info


def _cube_mesh(center, R, extent):
    from vmap_amd import meshing
    c = np.array([[x, y, z] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)]) * extent
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    v = c @ np.asarray(R).T + center
    return meshing.Mesh(torch.from_numpy(v.astype(np.float32)).to(DEV), torch.from_numpy(f.astype(np.int32)).to(DEV), None)


def test_the_box_drives_meshing_and_evaluation(scene):
    bounds, _ = _mods()
    from vmap_amd import evaluation, meshing
    from vmap_amd.trainer import SimpleConfig, Trainer
    _, objs = _store_scene(scene)
    bound = objs[0].get_bound(scene.k4)
    b = scene.boxes[0]
    A = meshing.bound_affine(bound, 0.9, 32)
    assert np.all(np.isfinite(np.asarray(A, np.float64)))
    torch.manual_seed(0)
    tr = Trainer(SimpleConfig(training_device=DEV, hidden_feature_size=32, obj_id=1))
    mesh = tr.meshing(bound, torch.tensor(bound.center, dtype=torch.float32, device=DEV), 32)      # an untrained field: a mesh or None, no error
    assert mesh is None or len(mesh.vertices) > 0
    gt = _cube_mesh(b["center"], b["R"], b["extent"])
    rec = _cube_mesh(b["center"], b["R"], b["extent"] * 1.02)
    m = evaluation.calc_3d_metric(rec, gt, N=5000, box=bound)
    assert m is not None and 0 < m[0][0] < 0.05 and m[3][0] > 0.9


def test_replica_frame_size():
    """20 keyframes of 1200 x 680, one object over about a fifth of each frame: conditions of the box on all its points, and
    obb_extents bit-identical under other launch geometries at that size."""
    bounds, _ = _mods()
    big = bo.Scene(width=1200, height=680, fx=1000.0, n_views=20, radius=3.0, seed=1)
    frac = np.mean([(f["inst"] == 3).mean() for f in big.frames])
    print(f"object 3 covers {frac:.3f} of a frame on average")
    assert 0.1 < frac < 0.35
    _, objs = _store_scene(big)
    box = objs[0].get_bound(big.k4)
    pts, off = bounds.object_points(objs[:1], big.k4)
    assert off[1] > 2_000_000
    assert bo.box_violations(box, pts.cpu().numpy()) == []
    rot = bo.random_rotations(np.random.default_rng(3), 1000).astype(np.float32)
    c = pts.mean(0, keepdim=True)
    lo, hi = bounds.extents(pts, rot, off, center=c)
    for chunks in (0, 3, 500):
        lo2, hi2 = bounds.extents(pts, rot, off, center=c, point_chunks=chunks)
        assert torch.equal(lo.view(torch.int32), lo2.view(torch.int32)) and torch.equal(hi.view(torch.int32), hi2.view(torch.int32)), chunks
