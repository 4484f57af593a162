"""GPU tier: one case per family pushed through the C ABI on the device AND through the CPU executor's wrappers (tests/simlib.py), so
that what the CPU tier runs is known to be what the device runs.  Integer and order outputs (mesh faces and counts, nearest-neighbour
indices, clip counts, unprojection offsets and point order) must be equal; float outputs are held to the tolerances of the existing
comparisons with the float64 checkers.  The executor's library is built by build() and loaded as it is."""
import numpy as np
import pytest
import torch

import bounds_oracle as bo
import simlib
from geom_checks import check_clip_against_oracle, check_mesh_against_oracle, check_nn, rotation_qr

pytestmark = pytest.mark.gpu


def test_mesh_device_and_executor_agree():
    from vmap_amd import meshing
    rng = np.random.default_rng(7)
    vol = rng.uniform(0, 1, (40, 31, 23)).astype(np.float32)
    A = np.array([[0.0, 0.05, 0.01, 1.0], [-0.04, 0.0, 0.02, -2.0], [0.01, 0.0, 0.07, 0.5]])
    for affine in (None, A):
        gv, gf, gn, _ = meshing.extract_mesh(torch.from_numpy(vol).cuda(), 0.5, affine).numpy()
        s = simlib.sim_mesh(vol, 0.5, affine)
        assert s["counts"].tolist() == [len(gv), len(gf)]
        np.testing.assert_array_equal(gf, s["faces"])
        for v, f, n in ((gv, gf, gn), (s["vertices"], s["faces"], s["normals"])):
            check_mesh_against_oracle(vol, v, f, n, affine)
        assert np.abs(gv - s["vertices"]).max() < 1e-5 * (1 if affine is None else np.abs(gv).max() + 1)


def test_evaluation_device_and_executor_agree():
    from vmap_amd import evaluation as ev
    from vmap_amd.meshing import BoundingBox, Mesh
    rng = np.random.default_rng(8)
    # nearest neighbours: three sets, one of them empty, refs over several tiles
    qs, rs = [700, 0, 2500], [1300, 40, 600]
    q = rng.uniform(-1, 1, (sum(qs), 3)).astype(np.float32)
    r = rng.uniform(-1, 1, (sum(rs), 3)).astype(np.float32)
    d, i = ev.nn_distance(q, r, qs, rs, return_index=True)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    qo, ro = np.concatenate([[0], np.cumsum(qs)]), np.concatenate([[0], np.cumsum(rs)])
    s = simlib.sim_nn(q, r, qo=qo, ro=ro)
    np.testing.assert_array_equal(i, s["index"])
    for k in (0, 2):
        for dist, idx in ((d, i), (s["dist"], s["index"])):
            check_nn(q[qo[k]:qo[k + 1]], r[ro[k]:ro[k + 1]], dist[qo[k]:qo[k + 1]], idx[qo[k]:qo[k + 1]] - ro[k])
    # cropping: the number of triangles, and each side against the float64 clipper
    centres = rng.uniform(2.5, 5.5, (1500, 1, 3))
    v = (centres + rng.normal(0, 0.12, (1500, 3, 3))).reshape(-1, 3).astype(np.float32)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)[rng.permutation(1500)]
    box = BoundingBox(center=[4.1, 3.9, 4.2], R=rotation_qr(rng), extent=[1.8, 1.2, 2.0])
    got = ev.crop_to_box(Mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), None), box)
    tri = got.vertices.cpu().numpy().reshape(-1, 3, 3)
    s = simlib.sim_clip(v, f, simlib.box15(box.center, box.R, box.extent))
    assert s["count"] == len(tri) == got.faces.shape[0]
    for t in (tri, s["triangles"]):
        check_clip_against_oracle(v, f, t, box.center, box.R, box.extent, min_inside=20)


def test_bounds_device_and_executor_agree():
    from test_gpu_bounds import _store_scene
    from vmap_amd import bounds
    scene = bo.Scene(width=80, height=60, fx=75.0, n_views=6, seed=3)
    store, objs = _store_scene(scene, extra_ids=(11,))
    pts, off = bounds.object_points(objs, scene.k4)
    pts = pts.cpu().numpy()
    n = len(scene.frames)
    pairs = np.array([(o.slots[k], o.obj_id) for o in objs for k in range(o.n_keyframes)], np.int32)        # what bounds.object_points hands the ABI
    assert len(pairs) == 3 * n
    s = simlib.sim_unproject(store.depth.cpu().numpy(), store.inst.cpu().numpy(), store.t_wc.cpu().numpy(), scene.k4, pairs,
                             np.array([0, n, 2 * n, 3 * n], np.int32))
    np.testing.assert_array_equal(np.asarray(off), s["offsets"])
    assert off[3] == off[2] and off[1] > 100
    for o, b in enumerate(scene.boxes):
        ref, scale = scene.cloud(b["id"])
        for p in (pts, s["points"]):                                   # the same points in the same order, each within the checker's bound
            assert (np.abs(p[off[o]:off[o + 1]].astype(np.float64) - ref) <= 6 * 2.0 ** -24 * scale).all()
    # extents of the two clouds along shared candidates, with a centre
    rng = np.random.default_rng(9)
    rot = bo.random_rotations(rng, 300).astype(np.float32)
    centre = np.stack([pts[off[o]:off[o + 1]].mean(0) if off[o + 1] > off[o] else np.zeros(3) for o in range(3)]).astype(np.float32)
    lo, hi = bounds.extents(torch.from_numpy(pts).cuda(), rot, np.asarray(off, np.int64), center=centre)
    slo, shi = simlib.sim_obb_extents(pts, np.asarray(off, np.int64), rot, centre)
    for a, b in ((lo.cpu().numpy(), hi.cpu().numpy()), (slo, shi)):
        assert (a[2] == np.inf).all() and (b[2] == -np.inf).all()
        for o in range(2):
            lo64, hi64, mlo, mhi = bo.extents64(pts[off[o]:off[o + 1]], rot, centre[o])
            assert (np.abs(a[o] - lo64) <= 2.0 ** -22 * mlo).all() and (np.abs(b[o] - hi64) <= 2.0 ** -22 * mhi).all()
