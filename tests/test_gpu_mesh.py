"""Mesh extraction, GPU tier: extract_mesh (vmapstep_mesh_count / _emit) against the numpy checker as arrays, Trainer.meshing against
the reference's pipeline written in torch, and a 256^3 sphere."""
import time

import numpy as np
import pytest
import torch

import mesh_oracle as mo
from conftest import load_golden
from geom_checks import check_mesh_against_oracle

pytestmark = pytest.mark.gpu

FIXTURES = ("sphere", "blob", "noncubic", "noise", "exact", "tiny")


def _random_volumes():
    rng = np.random.default_rng(7)
    for shape in ((2, 2, 2), (2, 5, 7), (3, 2, 9), (9, 11, 2), (17, 4, 33), (40, 31, 23), (64, 64, 64)):
        yield f"uniform{shape}", rng.uniform(0, 1, shape).astype(np.float32)
    # a smooth field over a non-cubic grid that spans several workgroups per row
    X, Y, Z = np.meshgrid(*[np.linspace(-1, 1, n) for n in (37, 50, 71)], indexing="ij")
    yield "smooth(37,50,71)", (1 / (1 + np.exp(-6 * (0.7 - np.sqrt(X ** 2 + (1.3 * Y) ** 2 + Z ** 2) + 0.1 * np.sin(7 * X))))).astype(np.float32)


def _volumes():
    for name in FIXTURES:
        yield f"fixture {name}", load_golden(f"mesh_{name}")["volume"]
    yield from _random_volumes()


def _check_against_oracle(vol, mesh, affine=None):
    gv, gf, gn, gc = mesh.numpy()
    assert gc is None and gn is not None
    check_mesh_against_oracle(vol, gv, gf, gn, affine)


@pytest.mark.parametrize("name,vol", list(_volumes()), ids=lambda x: x if isinstance(x, str) else "")
def test_extract_mesh_equals_oracle(name, vol):
    from vmap_amd import meshing
    t = torch.from_numpy(vol).cuda()
    m1 = meshing.extract_mesh(t)
    _, f, _, _ = mo.marching_cubes(vol)
    if len(f) == 0:
        assert m1 is None
        return
    _check_against_oracle(vol, m1)
    m2 = meshing.extract_mesh(t)
    for a, b in zip(m1.numpy()[:3], m2.numpy()[:3]):
        assert a.tobytes() == b.tobytes()          # bit-identical from call to call


@pytest.mark.parametrize("name", [n for n in FIXTURES if n != "exact"])
def test_extract_mesh_equals_skimage_lorensen_up_to_order(name):
    from vmap_amd import meshing
    g = load_golden(f"mesh_{name}")
    vol = g["volume"]
    gv, gf, _, _ = meshing.extract_mesh(torch.from_numpy(vol).cuda()).numpy()
    sid = mo.vertex_edge_ids(g["lorensen_vertices"], vol.shape)
    eid = mo.vertex_edge_ids(gv, vol.shape)
    assert (np.diff(eid) > 0).all()                 # the defined order: owning point, then axis
    np.testing.assert_array_equal(np.sort(sid), eid)
    np.testing.assert_array_equal(mo.canonical_faces(g["lorensen_faces"], sid), mo.canonical_faces(gf, eid))
    assert np.abs(g["lorensen_vertices"][np.argsort(sid)] - gv).max() < 1e-5


def test_extract_mesh_affine_and_level():
    from vmap_amd import meshing
    vol = load_golden("mesh_noncubic")["volume"]
    A = np.array([[0.0, 0.05, 0.01, 1.0], [-0.04, 0.0, 0.02, -2.0], [0.01, 0.0, 0.07, 0.5]])
    _check_against_oracle(vol, meshing.extract_mesh(torch.from_numpy(vol).cuda(), 0.5, A), A)
    t = torch.from_numpy(vol).cuda()
    for level in (float(vol.max()), float(vol.max()) + 1, float(vol.min()) - 1):
        assert meshing.extract_mesh(t, level) is None
    v, f, _, _ = mo.marching_cubes(vol, 0.3)
    m = meshing.extract_mesh(t, 0.3)
    np.testing.assert_array_equal(m.numpy()[1], f)
    # a non-contiguous view is meshed as its contiguous copy
    big = torch.from_numpy(np.ascontiguousarray(np.transpose(vol, (2, 0, 1)))).cuda().permute(1, 2, 0)
    np.testing.assert_array_equal(meshing.extract_mesh(big).numpy()[1], mo.marching_cubes(vol)[1])


def _rotation(a, b):
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return Rz @ Rx


def _trainer_with_surface(H, bound, obj_center):
    """A randomly initialised field whose occupancy crosses 0.5 inside the box: out_alpha's bias shifted by the median logit."""
    from vmap_amd.trainer import SimpleConfig, Trainer
    torch.manual_seed(H)
    tr = Trainer(SimpleConfig(training_device="cuda:0", hidden_feature_size=H, obj_id=0 if H == 128 else 1))
    pts = _reference_grid(tr, bound, obj_center, 32)
    with torch.no_grad():
        alpha, _ = tr.fc_occ_map(tr.pe(pts))
        tr.fc_occ_map.out_alpha.bias -= alpha.median() / 10.0      # the module scales the head by 10
    return tr


def _reference_grid(tr, bound, obj_center, D):
    """render_rays.make_3D_grid + trainer.py:36-49 in torch."""
    scale = torch.from_numpy(bound.extent / (2.0 * tr.bound_extent)).float().cuda()
    T = torch.eye(4)
    T[:3, 3] = torch.from_numpy(bound.center).float()
    T[:3, :3] = torch.from_numpy(bound.R).float()
    T = T.cuda()
    t = torch.linspace(-1.0, 1.0, steps=D, device="cuda")
    g = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1) * scale
    g = torch.stack([(T[None, None, None, r, :3] * g).sum(-1) for r in range(3)], -1) + T[None, None, None, :3, 3]
    return g.view(-1, 3) - obj_center.cuda()


def _reference_meshing(tr, bound, obj_center, D):
    pts = _reference_grid(tr, bound, obj_center, D)
    with torch.no_grad():
        occ = torch.cat([torch.sigmoid(tr.fc_occ_map(tr.pe(c))[0].squeeze(-1)) for c in pts.split(100000)])
    vol = occ.view(D, D, D).cpu().numpy()
    v, f, _, _ = mo.marching_cubes(vol)
    if len(f) == 0:
        return None
    scale = bound.extent / (2.0 * tr.bound_extent)
    v = ((v / (D - 1) - 0.5) * 2 * scale) @ bound.R.T + bound.center
    vt = torch.from_numpy(v).float().cuda()
    with torch.no_grad():
        col = tr.fc_occ_map(tr.pe(vt))[1]
    return v, f, (col * 255).cpu().numpy().astype(np.uint8)


@pytest.mark.parametrize("H", [32, 128])
@pytest.mark.parametrize("D", [64, 37])
def test_trainer_meshing_matches_reference_pipeline(H, D):
    from vmap_amd import meshing
    bound = meshing.BoundingBox(center=np.array([0.4, -0.3, 1.1]), R=_rotation(0.6, -0.35), extent=np.array([1.1, 0.7, 1.5]))
    obj_center = torch.tensor([0.05, -0.1, 0.2])
    tr = _trainer_with_surface(H, bound, obj_center)
    mesh = tr.meshing(bound, obj_center, D)
    assert mesh is not None
    gv, gf, gn, gc = mesh.numpy()
    assert gc.dtype == np.uint8 and gc.shape == gv.shape and gf.min() >= 0 and gf.max() < len(gv)
    if D == 64:
        assert len(gf) >= 1000
    # exact part: the mesh is the oracle's on the occupancy grid meshing queried, mapped to scene coordinates
    A_grid = meshing.bound_affine(bound, tr.bound_extent, D, obj_center)
    occ, _ = tr.eval_points(meshing.grid_points((D, D, D), A_grid))
    vol = occ.view(D, D, D).cpu().numpy()
    A = meshing.bound_affine(bound, tr.bound_extent, D)
    v, f, n, _ = mo.marching_cubes(vol, 0.5, A)
    np.testing.assert_array_equal(gf, f)
    assert np.abs(gv - v).max() < 1e-5 * (np.abs(v).max() + 1)
    # tolerance part: the reference pipeline in torch
    rv, rf, rc = _reference_meshing(tr, bound, obj_center, D)
    assert abs(len(rf) - len(gf)) <= 0.005 * len(rf)
    a, b = torch.from_numpy(gv).double().cuda(), torch.from_numpy(rv).double().cuda()
    d_ab = torch.cat([torch.cdist(x, b).min(1).values for x in a.split(4096)])
    d_ba = torch.cat([torch.cdist(x, a).min(1).values for x in b.split(4096)])
    hausdorff = max(d_ab.max().item(), d_ba.max().item())
    assert hausdorff <= 1e-3 * bound.extent.max(), hausdorff
    nearest = torch.cat([torch.cdist(x, b).argmin(1) for x in a.split(4096)]).cpu().numpy()
    close = np.abs(gc.astype(np.int32) - rc[nearest].astype(np.int32)).max(1) <= 1
    assert close.mean() >= 0.999, close.mean()


def test_trainer_meshing_returns_none_without_surface():
    from vmap_amd import meshing
    from vmap_amd.trainer import SimpleConfig, Trainer
    torch.manual_seed(0)
    tr = Trainer(SimpleConfig(training_device="cuda:0", hidden_feature_size=32, obj_id=1))
    bound = meshing.BoundingBox(extent=np.array([1.0, 1.0, 1.0]))
    with torch.no_grad():
        tr.fc_occ_map.out_alpha.bias.fill_(-3.0)       # logits -22 .. -48 (the head is scaled by 10): occupancy below 0.5, above 0
    assert tr.meshing(bound, torch.tensor(0.0), 24) is None
    with torch.no_grad():
        tr.fc_occ_map.out_alpha.bias.fill_(-1e3)       # occupancy exactly 0: eval_points itself returns None
    assert tr.meshing(bound, torch.tensor(0.0), 24) is None


def test_sphere_256_is_watertight():
    from vmap_amd import meshing
    D, r0 = 256, 0.6
    t = torch.linspace(-1, 1, D, device="cuda")
    X, Y, Z = torch.meshgrid(t, t, t, indexing="ij")
    vol = torch.sigmoid(20 * (r0 - torch.sqrt(X * X + Y * Y + Z * Z)))
    mesh = meshing.extract_mesh(vol)
    v, f, n, _ = mesh.numpy()
    assert f.min() >= 0 and f.max() < len(v)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64), 1)
    _, counts = np.unique(e[:, 0] * len(v) + e[:, 1], return_counts=True)
    assert (counts == 2).all()                               # every edge in exactly two faces
    assert len(v) - len(counts) + len(f) == 2                # Euler characteristic of a sphere
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum()
    r = r0 * (D - 1) / 2
    assert abs(area / (4 * np.pi * r * r) - 1) < 0.005
    # outward normals (towards decreasing occupancy)
    c = (D - 1) / 2
    assert ((v - c) * n).sum(1).min() > 0


def test_trainer_meshing_256():
    from vmap_amd import meshing
    bound = meshing.BoundingBox(center=np.array([0.1, 0.2, -0.3]), R=_rotation(0.3, 0.2), extent=np.array([1.2, 0.9, 1.0]))
    obj_center = torch.tensor([0.01, 0.02, 0.03])
    tr = _trainer_with_surface(32, bound, obj_center)
    tr.meshing(bound, obj_center, 64)                         # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh = tr.meshing(bound, obj_center, 256)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    v, f, _, c = mesh.numpy()
    print(f"\n[mesh] Trainer.meshing(grid_dim=256), hidden 32: {dt * 1e3:.1f} ms, {len(v)} vertices, {len(f)} faces")
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(v) and c.shape == v.shape
    # the mesh is the oracle's on the grid meshing queried
    A_grid = meshing.bound_affine(bound, tr.bound_extent, 256, obj_center)
    occ, _ = tr.eval_points(meshing.grid_points((256,) * 3, A_grid))
    _, of, _, _ = mo.marching_cubes(occ.view(256, 256, 256).cpu().numpy(), 0.5)
    np.testing.assert_array_equal(f, of)
