"""Mesh evaluation, GPU tier: vmapstep_nn_distance against the float64 brute force and scipy's recorded distances, batching and
determinism; vmapstep_surface_sample in test and Philox mode; vmapstep_clip_box_* against the float64 clipper; calc_3d_metric on
analytic spheres, against the float64 metrics of its own samples, and calc_3d_metrics against single calls."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_oracle as eo
from conftest import ROOT, load_golden
from geom_checks import check_clip_against_oracle, check_nn as _check_nn, rotation_qr, whole_triangle_case

pytestmark = pytest.mark.gpu

TILE, QB = 512, 2048            # the kernel's ref tile and queries per work item (csrc/eval_kernels.h)


def _ev():
    from vmap_amd import evaluation
    return evaluation


def _cloud(kind, n, rng, offset=0.0):
    if kind == "random":
        p = rng.uniform(-1, 1, (n, 3))
    else:
        c = rng.uniform(-1, 1, (8, 3))
        p = c[rng.integers(0, 8, n)] + rng.normal(0, 0.02, (n, 3))
    return (p + offset).astype(np.float32)


CASES = [(1, 1), (1, 700), (63, 64), (64, 65), (65, 63), (TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1), (QB - 1, 2 * TILE + 1),
         (QB + 1, 3 * TILE - 1), (3000, 2 * TILE)]


@pytest.mark.parametrize("kind", ["random", "clustered"])
@pytest.mark.parametrize("offset", [0.0, 5.0])
@pytest.mark.parametrize("n,m", CASES)
def test_nn_matches_float64_brute_force(kind, offset, n, m):
    rng = np.random.default_rng(n * 7919 + m + int(offset))
    q, r = _cloud(kind, n, rng, offset), _cloud(kind, m, rng, offset)
    d, i = _ev().nn_distance(q, r, return_index=True)
    _check_nn(q, r, d.cpu().numpy(), i.cpu().numpy())


@pytest.mark.parametrize("name", ["uniform", "clustered", "duplicates", "room5m"])
def test_nn_matches_ckdtree_fixtures(name):
    g = load_golden(f"eval_{name}")
    ev = _ev()
    L = max(np.abs(g["gt"]).max(), np.abs(g["rec"]).max())
    for q, r, d_ref in ((g["rec"], g["gt"], g["d_rec_gt"]), (g["gt"], g["rec"], g["d_gt_rec"])):
        d = ev.nn_distance(q, r).cpu().numpy().astype(np.float64)
        assert (np.abs(d - d_ref) <= 1e-6 * (d_ref + L)).all()
    m = [ev.accuracy(g["gt"], g["rec"]), ev.completion(g["gt"], g["rec"]), ev.completion_ratio(g["gt"], g["rec"], 0.01),
         ev.completion_ratio(g["gt"], g["rec"], 0.05)]
    np.testing.assert_allclose(m[:2], g["metrics"][:2], rtol=1e-6)
    np.testing.assert_allclose(m[2:], g["metrics"][2:], atol=2.0 / len(g["gt"]))
    assert abs(ev.chamfer(g["gt"], g["rec"]) - (g["metrics"][0] + g["metrics"][1]) / 2) < 1e-6 * g["metrics"][0]


def test_nn_large_sets():
    rng = np.random.default_rng(1)
    ev = _ev()
    q, r = _cloud("random", 10000, rng), _cloud("random", 10000, rng)
    d, i = ev.nn_distance(q, r, return_index=True)
    _check_nn(q, r, d.cpu().numpy(), i.cpu().numpy())
    # 200k queries x 20k refs, room scale: a sample of the queries against the brute force
    q, r = _cloud("clustered", 200000, rng, 5.0), _cloud("clustered", 20000, rng, 5.0)
    d, i = ev.nn_distance(q, r, return_index=True)
    pick = rng.choice(len(q), 3000, replace=False)
    _check_nn(q[pick], r, d.cpu().numpy()[pick], i.cpu().numpy()[pick])


def test_nn_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(2)
    base = rng.uniform(0, 1, (700, 3)).astype(np.float32)
    r = np.concatenate([base, base, base[::-1]])                  # every point three times; the first copy has the lowest index
    d, i = _ev().nn_distance(base, r, return_index=True)
    assert (d.cpu().numpy() == 0).all()
    np.testing.assert_array_equal(i.cpu().numpy(), np.arange(700))
    # equidistant refs around the query, in both index orders
    ring = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    for refs in (ring, ring[::-1].copy()):
        d, i = _ev().nn_distance(np.zeros((1, 3), np.float32), np.concatenate([np.full((TILE + 3, 3), 9, np.float32), refs]), return_index=True)
        assert float(d[0]) == 1.0 and int(i[0]) == TILE + 3


def _segmented_case(rng):
    qs, rs = [], []
    for s in range(100):
        kind = s % 5
        nq = [0, 1, int(rng.integers(2, 3000)), 10000, int(rng.integers(2000, 12000))][kind]
        nr = [0 if s % 10 == 0 else 5, int(rng.integers(1, 100)), int(rng.integers(500, 3000)), 10000, int(rng.integers(1, 12000))][kind]
        qs.append(nq)
        rs.append(nr)
    q = _cloud("random", sum(qs), rng, 3.0)
    r = _cloud("random", sum(rs), rng, 3.0)
    return q, r, qs, rs


def test_nn_segmented_batch_equals_single_calls_and_is_deterministic():
    rng = np.random.default_rng(3)
    ev = _ev()
    q, r, qs, rs = _segmented_case(rng)
    d, i = ev.nn_distance(q, r, qs, rs, return_index=True)
    d2, i2 = ev.nn_distance(q, r, qs, rs, return_index=True)
    assert torch.equal(d, d2) and torch.equal(i, i2)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    qo, ro = np.concatenate([[0], np.cumsum(qs)]), np.concatenate([[0], np.cumsum(rs)])
    for s in range(100):
        if qs[s] == 0:
            continue
        ds, is_ = ev.nn_distance(q[qo[s]:qo[s + 1]], r[ro[s]:ro[s + 1]], return_index=True)
        np.testing.assert_array_equal(d[qo[s]:qo[s + 1]], ds.cpu().numpy())
        np.testing.assert_array_equal(i[qo[s]:qo[s + 1]], is_.cpu().numpy() + ro[s])
    # spot checks against the brute force
    for s in (2, 3, 17, 54):
        _check_nn(q[qo[s]:qo[s + 1]], r[ro[s]:ro[s + 1]], d[qo[s]:qo[s + 1]], i[qo[s]:qo[s + 1]] - ro[s])


def test_nn_over_more_sets_than_one_plan_chunk_equals_single_calls():
    """1025 small sets, some without queries or without anything: nn_plan's prefix of the work items leaves its first chunk of 1024
    sets, and nn_search finds the set of every item in it.  Against the same call made set by set, bit for bit."""
    rng = np.random.default_rng(31)
    ev = _ev()
    n_sets = 1025
    qs = rng.integers(1, 40, n_sets)
    rs = rng.integers(1, 30, n_sets)
    empty = rng.random(n_sets) < 0.2
    empty[[0, 511, 1023]] = True                                   # an empty set first and on both sides of the chunk's edge
    empty[[1, 1022, 1024]] = False
    qs[empty] = 0
    rs[empty & (rng.random(n_sets) < 0.5)] = 0                     # refs without queries, or nothing at all
    q = _cloud("random", int(qs.sum()), rng, 3.0)
    r = _cloud("random", int(rs.sum()), rng, 3.0)
    d, i = ev.nn_distance(q, r, qs, rs, return_index=True)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    qo, ro = np.concatenate([[0], np.cumsum(qs)]), np.concatenate([[0], np.cumsum(rs)])
    assert (qs[1024] > 0) and len(d) == qo[-1]
    for s in range(n_sets):
        if qs[s] == 0:
            continue
        ds, is_ = ev.nn_distance(q[qo[s]:qo[s + 1]], r[ro[s]:ro[s + 1]], return_index=True)
        np.testing.assert_array_equal(d[qo[s]:qo[s + 1]], ds.cpu().numpy(), err_msg=f"set {s}")
        np.testing.assert_array_equal(i[qo[s]:qo[s + 1]], is_.cpu().numpy() + ro[s], err_msg=f"set {s}")
    for s in (1, 1022, 1024):
        _check_nn(q[qo[s]:qo[s + 1]], r[ro[s]:ro[s + 1]], d[qo[s]:qo[s + 1]], i[qo[s]:qo[s + 1]] - ro[s])


def test_nn_writes_only_its_query_range():
    rng = np.random.default_rng(4)
    ev = _ev()
    from vmap_amd import _lib
    import ctypes
    lib = _lib.load()
    q = torch.from_numpy(_cloud("random", 5000, rng)).cuda()
    r = torch.from_numpy(_cloud("random", 3000, rng)).cuda()
    qo_h = np.array([100, 100, 2100, 4000], np.int64)             # queries [0, 100) and [4000, 5000) belong to no set
    ro_h = np.array([0, 7, 1500, 3000], np.int64)
    qo_d, ro_d = torch.from_numpy(qo_h).cuda(), torch.from_numpy(ro_h).cuda()
    dist = torch.full((5000,), -7.0, device="cuda")
    nb = ctypes.c_size_t()
    assert lib.vmapstep_nn_workspace_bytes(5000, 3, ctypes.byref(nb)) == 0
    ws = torch.empty(nb.value + 256, dtype=torch.uint8, device="cuda")
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))         # noqa: E731
    _lib.check(lib.vmapstep_nn_distance(q.data_ptr(), 5000, qo_d.data_ptr(), p(qo_h), r.data_ptr(), 3000, ro_d.data_ptr(), p(ro_h), 3,
                                        dist.data_ptr(), None, wp, nb.value, torch.cuda.current_stream().cuda_stream), lib)
    d = dist.cpu().numpy()
    assert (d[:100] == -7).all() and (d[4000:] == -7).all()
    np.testing.assert_array_equal(d[100:2100], ev.nn_distance(q[100:2100], r[7:1500]).cpu().numpy())
    np.testing.assert_array_equal(d[2100:4000], ev.nn_distance(q[2100:4000], r[1500:]).cpu().numpy())


def _random_mesh(rng, nv=300, nf=800, scale=1.0, offset=0.0):
    from vmap_amd.meshing import Mesh
    v = (rng.uniform(-1, 1, (nv, 3)) * scale + offset).astype(np.float32)
    f = rng.integers(0, nv, (nf, 3)).astype(np.int32)
    return Mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), None), v, f


def test_sampling_test_mode_matches_the_formula():
    rng = np.random.default_rng(5)
    ev = _ev()
    meshes, counts, u0s, rs, want_pts, want_face = [], [], [], [], [], []
    for s, (nf, n) in enumerate([(800, 3000), (1, 50), (5000, 7000)]):
        m, v, f = _random_mesh(rng, nf=nf, offset=2.0 * s)
        area = eo.face_areas(v, f)
        cdf = np.cumsum(area)
        face = rng.choice(np.flatnonzero(area > 1e-3 * area.max()), n)      # faces with an interval of their own on the CDF
        lo = np.where(face > 0, cdf[face - 1], 0.0)
        u0 = (lo + (0.25 + 0.5 * rng.uniform(size=n)) * (cdf[face] - lo)) / cdf[-1]         # away from the CDF's steps
        r = rng.uniform(0, 1, (n, 2)).astype(np.float32)
        p, fc = eo.sample(v, f, u0, r)
        np.testing.assert_array_equal(fc, face)
        meshes.append(m), counts.append(n), u0s.append(u0), rs.append(r), want_pts.append(p), want_face.append(fc)
    pts, fidx = ev._sample_sets(meshes, counts, randoms=(torch.from_numpy(np.concatenate(u0s)).cuda(), torch.from_numpy(np.concatenate(rs)).cuda()),
                                return_face_index=True)
    want = np.concatenate(want_pts)
    L = np.abs(want).max()
    assert np.abs(pts.cpu().numpy() - want).max() <= 1e-6 * L
    np.testing.assert_array_equal(fidx.cpu().numpy(), np.concatenate(want_face))


def test_sampling_philox_mode():
    rng = np.random.default_rng(6)
    ev = _ev()
    m, v, f = _random_mesh(rng, nv=40, nf=60)
    n = 400000
    pts, fidx = ev._sample_sets([m], [n], seed=123, return_face_index=True)
    p, fi = pts.cpu().numpy().astype(np.float64), fidx.cpu().numpy()
    # every point on its face: barycentric coordinates in [0, 1] and on the plane
    v64 = v.astype(np.float64)
    a, b, c = v64[f[fi, 0]], v64[f[fi, 1]], v64[f[fi, 2]]
    e1, e2, w = b - a, c - a, p - a
    nrm = np.cross(e1, e2)
    big = np.linalg.norm(nrm, axis=1) > 1e-3
    assert (np.abs((w * nrm).sum(1)[big]) / np.linalg.norm(nrm, axis=1)[big] < 1e-5).all()
    G = np.stack([np.stack([(e1 * e1).sum(1), (e1 * e2).sum(1)], 1), np.stack([(e1 * e2).sum(1), (e2 * e2).sum(1)], 1)], 1)
    rhs = np.stack([(w * e1).sum(1), (w * e2).sum(1)], 1)
    good = big & (np.abs(np.linalg.det(G)) > 1e-4)
    bary = np.linalg.solve(G[good], rhs[good][..., None])[..., 0]
    assert (bary > -1e-4).all() and (bary.sum(1) < 1 + 1e-4).all()
    # per-face hit counts: within 5 sigma of the area fractions
    area = eo.face_areas(v, f)
    prob = area / area.sum()
    hits = np.bincount(fi, minlength=len(f))
    sigma = np.sqrt(n * prob * (1 - prob))
    assert (np.abs(hits - n * prob) <= 5 * sigma + 1).all()
    # the same seed: the same bits; another seed, stream or set: other points
    again = ev._sample_sets([m], [n], seed=123)
    assert torch.equal(again, pts)
    for kw in (dict(seed=124), dict(seed=123, stream_id=1), dict(seed=123, set_base=1)):
        other = ev._sample_sets([m], [n], **kw)
        assert (other != pts).any(1).float().mean() > 0.99
    # a set sampled inside a batch draws the stream it draws alone at the same set number
    m2, _, _ = _random_mesh(rng)
    both = ev._sample_sets([m2, m], [1000, n], seed=123, set_base=4)
    assert torch.equal(both[1000:], ev._sample_sets([m], [n], seed=123, set_base=5))


def test_sampling_philox_mode_is_predicted_by_the_replica():
    """_sample_sets drawing its own numbers, at the sizes of the executor's test (sets of 60 and 1500 faces, 300 and 900 points, a
    64-bit seed, stream and set_base not zero): the faces eval_oracle.sample picks from philox_ref.surface_randoms, exactly, and its
    points."""
    from philox_ref import surface_randoms
    rng = np.random.default_rng(6)
    ev = _ev()
    sets = [_random_mesh(rng, nv=40, nf=60, offset=2.0), _random_mesh(rng, nv=40, nf=1500, offset=2.0)]
    counts = [300, 900]
    seed, stream, set_base = 0x1234_5678_9ABC_DEF0, 3, 4
    pts, fidx = ev._sample_sets([m for m, _, _ in sets], counts, seed=seed, stream_id=stream, set_base=set_base, return_face_index=True)
    pts, fidx = pts.cpu().numpy(), fidx.cpu().numpy()
    oo = np.concatenate([[0], np.cumsum(counts)])
    for s, (_, v, f) in enumerate(sets):
        u0, r = surface_randoms(counts[s], set_base + s, stream, seed)
        p, fc = eo.sample(v, f, u0, r)
        np.testing.assert_array_equal(fidx[oo[s]:oo[s + 1]], fc)
        assert np.abs(pts[oo[s]:oo[s + 1]] - p).max() <= 1e-6 * np.abs(p).max()


_rotation = rotation_qr


def test_clip_matches_the_float64_clipper():
    rng = np.random.default_rng(7)
    ev = _ev()
    from vmap_amd.meshing import BoundingBox
    # small triangles scattered over a 3 m cube around (4, 4, 4)
    from vmap_amd.meshing import Mesh
    centres = rng.uniform(2.5, 5.5, (6000, 1, 3))
    v = (centres + rng.normal(0, 0.12, (6000, 3, 3))).reshape(-1, 3).astype(np.float32)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)[rng.permutation(6000)]
    m = Mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), None)
    box = BoundingBox(center=[4.1, 3.9, 4.2], R=_rotation(rng), extent=[1.8, 1.2, 2.0])
    got = ev.crop_to_box(m, box)
    assert got.faces.shape[0] == got.vertices.shape[0] // 3
    check_clip_against_oracle(v, f, got.vertices.cpu().numpy().reshape(-1, 3, 3), box.center, box.R, box.extent)
    # everything outside: None; and determinism
    assert ev.crop_to_box(m, BoundingBox(center=[40, 40, 40], R=np.eye(3), extent=[1, 1, 1])) is None
    assert torch.equal(ev.crop_to_box(m, box).vertices, got.vertices)


@pytest.mark.parametrize("nblk", [1023, 1024, 1025, 2049])
def test_clip_of_whole_triangles_across_scan_chunks(nblk):
    """``nblk`` blocks of 256 faces (the last one partial), so that clip_scan ends on, at and past its chunks of 1024 block totals.
    Every triangle lies wholly inside the box or wholly beyond one of its planes, so the crop is v[f[inside]] bit for bit, in face
    order.  Runs of whole blocks keep nothing: totals of zero inside the scan."""
    ev = _ev()
    from vmap_amd.meshing import BoundingBox, Mesh
    v, f, inside, R, centre, extent = whole_triangle_case(nblk)
    got = ev.crop_to_box(Mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), None), BoundingBox(center=centre, R=R, extent=extent))
    assert got.faces.shape[0] == inside.sum()
    np.testing.assert_array_equal(got.vertices.cpu().numpy().reshape(-1, 3, 3), v[f[inside]])
    np.testing.assert_array_equal(got.faces.cpu().numpy(), np.arange(3 * inside.sum(), dtype=np.int32).reshape(-1, 3))


def _sphere_mesh(r, grid=256, center=(0.0, 0.0, 0.0)):
    from vmap_amd import meshing
    t = torch.linspace(-1, 1, grid, device="cuda", dtype=torch.float32)
    X, Y, Z = torch.meshgrid(t, t, t, indexing="ij")
    vol = (r - torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) + 0.5).contiguous()
    h = 2.0 / (grid - 1)
    aff = np.array([[h, 0, 0, -1 + center[0]], [0, h, 0, -1 + center[1]], [0, 0, h, -1 + center[2]]])
    return meshing.extract_mesh(vol, 0.5, aff)


def test_metrics_of_concentric_spheres():
    ev = _ev()
    from vmap_amd.meshing import BoundingBox, Mesh
    r, delta = 0.5, 0.02
    gt, rec = _sphere_mesh(r), _sphere_mesh(r + delta)
    box = BoundingBox(center=[0, 0, 0], R=np.eye(3), extent=[2 * r, 2 * r, 2 * r])
    m = ev.calc_3d_metric(rec, gt, N=200000, box=box)
    acc, comp, r1, r5 = (x[0] for x in m)
    assert abs(acc - delta) < 2e-3 and abs(comp - delta) < 2e-3
    assert r1 == 0.0 and r5 == 1.0
    assert ev.completion_ratio(*_points_pair(ev, gt, rec), dist_th=0.019) == 0.0
    assert ev.completion_ratio(*_points_pair(ev, gt, rec), dist_th=0.025) == 1.0
    # the default box (principal axes of the GT vertices) keeps the whole rec sphere here
    assert ev.calc_3d_metric(rec, gt, N=20000)[0][0] == pytest.approx(delta, abs=2e-3)
    # a mesh against itself: near zero, shrinking as N grows
    a_small = ev.calc_3d_metric(gt, gt, N=10000, box=box)[0][0]
    a_big = ev.calc_3d_metric(gt, gt, N=160000, box=box)[0][0]
    assert a_big < 0.5 * a_small and a_big < 3e-3
    # a far-away blob on the rec is cropped away by the box
    blob = _sphere_mesh(0.1, grid=64)
    far = Mesh(torch.cat([rec.vertices, blob.vertices + torch.tensor([3.0, 0, 0], device="cuda")]),
               torch.cat([rec.faces, blob.faces + len(rec.vertices)]), None)
    m2 = ev.calc_3d_metric(far, gt, N=200000, box=box)
    assert abs(m2[0][0] - delta) < 2e-3
    moved = Mesh(blob.vertices + torch.tensor([3.0, 0, 0], device="cuda"), blob.faces, None)
    assert ev.calc_3d_metric(moved, gt, N=1000, box=box) is None


def _points_pair(ev, gt, rec, n=200000):
    return ev.sample_surface(gt, n, seed=9, stream_id=1), ev.sample_surface(rec, n, seed=9)


def test_calc_3d_metric_equals_float64_metrics_of_its_samples():
    ev = _ev()
    from vmap_amd.meshing import BoundingBox
    gt = _sphere_mesh(0.4, grid=96)
    rec = _sphere_mesh(0.41, grid=80, center=(0.02, -0.01, 0.0))
    box = BoundingBox(center=[0.1, 0, 0], R=_rotation(np.random.default_rng(8)), extent=[0.7, 0.9, 0.8])
    N = 6000
    m = ev.calc_3d_metric(rec, gt, N=N, box=box, seed=5, index=3)
    crop = ev.crop_to_box(rec, ev._enlarged(box))
    rec_pts = ev.sample_surface(crop, N, seed=5, stream_id=0, set_index=3).cpu().numpy()
    gt_pts = ev.sample_surface(gt, N, seed=5, stream_id=1, set_index=3).cpu().numpy()
    want = eo.metrics(gt_pts, rec_pts)
    np.testing.assert_allclose([m[0][0], m[1][0]], [want[0][0], want[1][0]], rtol=1e-5)
    assert abs(m[2][0] - want[2][0]) <= 2.0 / N and abs(m[3][0] - want[3][0]) <= 2.0 / N


def test_calc_3d_metrics_equals_single_calls():
    ev = _ev()
    from vmap_amd.meshing import BoundingBox
    rng = np.random.default_rng(9)
    pairs = []
    for k in range(50):
        c = rng.uniform(-0.3, 0.3, 3)
        gt = _sphere_mesh(0.2 + 0.01 * (k % 7), grid=40, center=tuple(c))
        rec = _sphere_mesh(0.21 + 0.01 * (k % 5), grid=36, center=tuple(c + rng.normal(0, 0.01, 3)))
        box = None if k % 3 else BoundingBox(center=c, R=np.eye(3), extent=[0.5, 0.5, 0.5])
        if k == 17:                 # cropped to nothing
            box = BoundingBox(center=c + 5, R=np.eye(3), extent=[0.1, 0.1, 0.1])
        pairs.append((rec, gt, box))
    batch = ev.calc_3d_metrics(pairs, N=10000, seed=2)
    assert batch[17] is None and sum(x is None for x in batch) == 1
    for k, (rec, gt, box) in enumerate(pairs):
        single = ev.calc_3d_metric(rec, gt, N=10000, box=box, seed=2, index=k)
        if single is None:
            assert batch[k] is None
            continue
        np.testing.assert_allclose(np.array(batch[k]), np.array(single), rtol=1e-12, atol=0)
        assert 0.0 < batch[k][0][0] < 0.1


def test_cli_prints_one_json_line(tmp_path):
    gt = _sphere_mesh(0.3, grid=64)
    rec = _sphere_mesh(0.31, grid=64)
    gt.export(tmp_path / "gt.ply")
    rec.export(tmp_path / "rec.obj")
    out = subprocess.run([sys.executable, "-m", "vmap_amd.evaluation", str(tmp_path / "rec.obj"), str(tmp_path / "gt.ply"), "--n", "20000"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300, env={**os.environ, "PYTHONPATH": ROOT})
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()
    assert len(line) == 1
    res = json.loads(line[0])
    assert abs(res["accuracy"] - 0.01) < 3e-3 and abs(res["completion"] - 0.01) < 3e-3
    assert res["completion_ratio_5cm"] == 1.0
