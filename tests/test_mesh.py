"""Mesh extraction, CPU tier: the numpy checker (tests/mesh_oracle.py) against scikit-image's own output on the fixtures of
tests/golden/mesh_*.npz (make_mesh_goldens.py), the reference's transform chain, Mesh.export, and the argument checks of the
vmapstep_mesh_* entry points (no kernel is launched here)."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_oracle as mo
from conftest import load_golden
from vmap_amd import _lib, meshing

VOLUMES = ("sphere", "blob", "noncubic", "noise", "exact", "tiny")
SMOOTH = ("sphere", "blob", "noncubic")
AMBIGUOUS_CASES = (3, 4, 6, 7, 10, 12, 13)      # Lewiner's cases with an ambiguous face or interior


def _on_edges(v):
    """True iff every vertex has exactly one non-integer coordinate (no vertex at a grid point)."""
    return bool(((np.abs(v - np.round(v)) > 1e-6).sum(1) == 1).all())


def _position_faces(v, f):
    """Faces as rows of rounded vertex positions, rotated so the smallest vertex comes first (winding kept), rows sorted."""
    p = np.round(np.asarray(v, np.float64), 4)[np.asarray(f, np.int64)]          # [F,3,3]
    keys = [tuple(map(tuple, tri)) for tri in p]
    out = []
    for k in keys:
        r = min(range(3), key=lambda s: k[s])
        out.append(k[r:] + k[:r])
    return sorted(out)


@pytest.mark.parametrize("name", VOLUMES)
def test_oracle_equals_skimage_lorensen(name):
    g = load_golden(f"mesh_{name}")
    vol = g["volume"]
    v, f, n, eid = mo.marching_cubes(vol)
    sv, sf = g["lorensen_vertices"], g["lorensen_faces"]
    assert len(v) == len(sv) and len(f) == len(sf)
    if _on_edges(sv):
        sid = mo.vertex_edge_ids(sv, vol.shape)
        order = np.argsort(sid)
        np.testing.assert_array_equal(sid[order], eid)
        assert np.abs(sv[order] - v).max() < 1e-5
        np.testing.assert_array_equal(mo.canonical_faces(sf, sid), mo.canonical_faces(f, eid))
    else:
        # vertices at grid points (corner values exactly at the level): several edges can share a position; compare multisets
        assert name == "exact"
        np.testing.assert_allclose(np.sort(np.round(sv, 4), 0), np.sort(np.round(v, 4), 0), atol=1e-5)
        assert _position_faces(sv, sf) == _position_faces(v, f)


def _cell_of(v, f, shape):
    """The cell of each triangle: floor of its centroid (triangles of one cell lie in that closed cell)."""
    c = np.asarray(v, np.float64)[np.asarray(f, np.int64)].mean(1)
    c = np.clip(np.floor(c).astype(np.int64), 0, np.array(shape) - 2)
    return np.ravel_multi_index(tuple(c.T), tuple(np.array(shape) - 1))


@pytest.mark.parametrize("name", ("sphere", "blob", "noncubic", "noise"))
def test_oracle_against_skimage_lewiner(name, capsys):
    """Same edge vertices; triangles differ only in cells whose classic configuration is ambiguous (Lewiner may add a vertex inside
    such a cell)."""
    g = load_golden(f"mesh_{name}")
    vol = g["volume"]
    v, f, _, eid = mo.marching_cubes(vol)
    lv, lf = g["lewiner_vertices"], g["lewiner_faces"]
    interior = (np.abs(lv - np.round(lv)) > 1e-6).sum(1) != 1
    lid = mo.vertex_edge_ids(lv, vol.shape)
    np.testing.assert_array_equal(np.sort(lid[~interior]), eid)
    lid[interior] = -1 - np.arange(interior.sum())            # unique ids of Lewiner's cell-interior vertices
    ours = {}
    for cell, tri in zip(_cell_of(v, f, vol.shape), eid[f]):
        ours.setdefault(int(cell), []).append(tuple(np.roll(tri, -int(np.argmin(tri)))))
    theirs = {}
    for cell, tri in zip(_cell_of(lv, lf, vol.shape), lid[lf]):
        theirs.setdefault(int(cell), []).append(tuple(np.roll(tri, -int(np.argmin(tri)))))
    differ = sorted(c for c in set(ours) | set(theirs) if sorted(ours.get(c, [])) != sorted(theirs.get(c, [])))
    cube = np.zeros(np.array(vol.shape) - 1, np.int64)
    nx, ny, nz = vol.shape
    for c, (di, dj, dk) in enumerate(mo.CORNERS):
        cube |= (vol[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk] > 0.5).astype(np.int64) << c
    cases = g["lewiner_case"][cube.reshape(-1)[differ]]
    with capsys.disabled():
        print(f"\n[mesh] {name}: {len(differ)} of {len(ours)} cells triangulated differently by Lewiner (cases {sorted(set(cases.tolist()))}), "
              f"{int(interior.sum())} Lewiner interior vertices")
    assert np.isin(cases, AMBIGUOUS_CASES).all(), (differ, cases)
    if name != "noise":
        assert not differ


@pytest.mark.parametrize("name", SMOOTH)
def test_oracle_normals_follow_skimage_on_smooth_fields(name):
    g = load_golden(f"mesh_{name}")
    vol = g["volume"]
    _, _, n, eid = mo.marching_cubes(vol)
    sid = mo.vertex_edge_ids(g["lorensen_vertices"], vol.shape)
    sn = g["lorensen_normals"][np.argsort(sid)]
    assert (n * sn).sum(1).min() > 0.98


def test_exact_level_corners_and_level_out_of_range():
    vol = load_golden("mesh_exact")["volume"]
    assert (vol == 0.5).sum() > 10
    v, f, _, eid = mo.marching_cubes(vol)
    # a corner at exactly the level is not above it: the edge from it to a lower value carries no vertex
    pt, ax = eid // 3, eid % 3
    idx = np.stack(np.unravel_index(pt, vol.shape), -1)
    idx1 = idx.copy()
    idx1[np.arange(len(idx)), ax] += 1
    assert (np.maximum(vol[tuple(idx.T)], vol[tuple(idx1.T)]) > 0.5).all()
    for level in (float(vol.max()), float(vol.max()) + 0.1, float(vol.min()) - 0.1):
        v, f, _, _ = mo.marching_cubes(vol, level)
        assert len(f) == 0 and len(v) == 0


def test_tiny_volume():
    g = load_golden("mesh_tiny")
    v, f, _, _ = mo.marching_cubes(g["volume"])
    assert len(f) == len(g["lorensen_faces"]) > 0 and f.max() < len(v)


def test_transform_chain_matches_the_reference():
    g = load_golden("mesh_transform")
    D = int(g["D"])
    bound = meshing.BoundingBox(center=g["center"], R=g["R"], extent=g["extent"])
    A = meshing.bound_affine(bound, float(g["bound_extent"]), D, torch.tensor(g["obj_center"]))
    idx = np.stack(np.meshgrid(*[np.arange(D)] * 3, indexing="ij"), -1).reshape(-1, 3)
    np.testing.assert_allclose(idx @ A[:, :3].T + A[:, 3], g["grid"], atol=1e-12)
    A = meshing.bound_affine(bound, float(g["bound_extent"]), D)
    np.testing.assert_allclose(g["v_index"] @ A[:, :3].T + A[:, 3], g["v_scene"], atol=1e-12)


def _read_obj(path):
    v, c, n, f = [], [], [], []
    for line in open(path):
        t = line.split()
        if t[0] == "v":
            v.append([float(x) for x in t[1:4]])
            c.append([float(x) for x in t[4:7]])
        elif t[0] == "vn":
            n.append([float(x) for x in t[1:4]])
        elif t[0] == "f":
            a = [s.split("//") for s in t[1:]]
            assert all(p == q for p, q in a)
            f.append([int(p) - 1 for p, _ in a])
    return np.array(v), np.array(c), np.array(n), np.array(f)


def _read_ply(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    nv = int(next(s for s in lines if s.startswith("element vertex")).split()[-1])
    nf = int(next(s for s in lines if s.startswith("element face")).split()[-1])
    props = [s.split()[1:] for s in lines if s.startswith("property") and "list" not in s]
    dt = np.dtype([(name, "<f4" if ty == "float" else "u1") for ty, name in props])
    vert = np.frombuffer(body, dt, nv)
    face = np.frombuffer(body[nv * dt.itemsize:], np.dtype([("k", "u1"), ("i", "<i4", 3)]), nf)
    assert (face["k"] == 3).all()
    return vert, face["i"]


def test_export_round_trips(tmp_path):
    vol = load_golden("mesh_blob")["volume"]
    v, f, n, _ = mo.marching_cubes(vol)
    c = (np.arange(3 * len(v)) % 256).astype(np.uint8).reshape(-1, 3)
    mesh = meshing.Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(c))
    mesh.export(tmp_path / "m.obj")
    ov, oc, on, of = _read_obj(tmp_path / "m.obj")
    np.testing.assert_allclose(ov, v, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(on, n, rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(np.round(oc * 255).astype(np.uint8), c)
    np.testing.assert_array_equal(of, f)
    mesh.export(tmp_path / "m.ply")
    pv, pf = _read_ply(tmp_path / "m.ply")
    np.testing.assert_array_equal(np.stack([pv["x"], pv["y"], pv["z"]], 1), v)
    np.testing.assert_array_equal(np.stack([pv["nx"], pv["ny"], pv["nz"]], 1), n)
    np.testing.assert_array_equal(np.stack([pv["red"], pv["green"], pv["blue"]], 1), c)
    np.testing.assert_array_equal(pf, f)
    with pytest.raises(ValueError):
        mesh.export(tmp_path / "m.stl")


def test_mesh_abi_argument_checks():
    lib = _lib.load()
    nb = ctypes.c_size_t()
    assert lib.vmapstep_mesh_workspace_bytes(2, 2, 2, ctypes.byref(nb)) == 0 and nb.value > 0 and nb.value % 256 == 0
    assert lib.vmapstep_mesh_workspace_bytes(256, 256, 256, ctypes.byref(nb)) == 0
    assert nb.value >= 256 ** 3 * 5 + (256 ** 3 // 256) * 16
    assert lib.vmapstep_mesh_workspace_bytes(2, 2, 2, None) == -1
    for shape in ((1, 4, 4), (4, 4, 1), (0, 2, 2), (1025, 2, 2), (1024, 1024, 700)):
        assert lib.vmapstep_mesh_workspace_bytes(*shape, ctypes.byref(nb)) == -2, shape
    assert b"2..1024" in lib.vmapstep_last_error()
    aff = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    counts = ctypes.c_void_p(16)          # never dereferenced: every call below fails its checks first
    vol = ctypes.c_void_p(16)
    assert lib.vmapstep_mesh_grid_points(8, 8, 8, None, vol, None) == -1
    assert lib.vmapstep_mesh_grid_points(8, 8, 8, aff, None, None) == -1
    assert lib.vmapstep_mesh_grid_points(8, 1, 8, aff, vol, None) == -2
    assert lib.vmapstep_mesh_count(None, 8, 8, 8, 0.5, counts, None, 0, None) == -1
    assert lib.vmapstep_mesh_count(vol, 8, 8, 8, 0.5, None, None, 0, None) == -1
    assert lib.vmapstep_mesh_count(vol, 8, 8, 2000, 0.5, counts, None, 0, None) == -2
    assert lib.vmapstep_mesh_workspace_bytes(8, 8, 8, ctypes.byref(nb)) == 0
    assert lib.vmapstep_mesh_count(vol, 8, 8, 8, 0.5, counts, None, nb.value, None) == -3
    assert lib.vmapstep_mesh_count(vol, 8, 8, 8, 0.5, counts, ctypes.c_void_p(256 * 7), nb.value - 1, None) == -3
    assert lib.vmapstep_mesh_count(vol, 8, 8, 8, 0.5, counts, ctypes.c_void_p(256 * 7 + 4), nb.value, None) == -3
    assert b"workspace" in lib.vmapstep_last_error()
    ws = ctypes.c_void_p(256 * 7)
    assert lib.vmapstep_mesh_emit(None, 8, 8, 8, 0.5, None, vol, None, vol, 10, 10, ws, nb.value, None) == -1
    assert lib.vmapstep_mesh_emit(vol, 8, 8, 8, 0.5, None, None, None, vol, 10, 10, ws, nb.value, None) == -1
    assert lib.vmapstep_mesh_emit(vol, 8, 8, 8, 0.5, None, vol, None, None, 10, 10, ws, nb.value, None) == -1
    assert lib.vmapstep_mesh_emit(vol, 8, 8, 8, 0.5, None, vol, None, vol, -1, 10, ws, nb.value, None) == -1
    assert lib.vmapstep_mesh_emit(vol, 8, 8, 1, 0.5, None, vol, None, vol, 10, 10, ws, nb.value, None) == -2
    assert lib.vmapstep_mesh_emit(vol, 8, 8, 8, 0.5, None, vol, None, vol, 10, 10, ws, nb.value - 1, None) == -3
    singular = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0)
    assert lib.vmapstep_mesh_emit(vol, 8, 8, 8, 0.5, singular, vol, None, vol, 10, 10, ws, nb.value, None) == -1
    assert b"singular" in lib.vmapstep_last_error()
    # nothing to write: accepted without touching the device
    assert lib.vmapstep_mesh_emit(vol, 8, 8, 8, 0.5, aff, None, None, None, 0, 0, ws, nb.value, None) == 0


def test_extract_mesh_refuses_host_tensors():
    with pytest.raises(_lib.VmapStepError):
        meshing.extract_mesh(torch.zeros(4, 4, 4))
