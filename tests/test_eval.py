"""Mesh evaluation, CPU tier: the numpy checker (tests/eval_oracle.py) against scipy's cKDTree as recorded in tests/golden/eval_*.npz
(make_eval_goldens.py) and live where scipy exists, the clipper on analytic cases, load_mesh, the principal-axes box, and the argument
checks of the vmapstep_nn / surface_sample / clip_box entry points (no kernel is launched here)."""
import ctypes

import numpy as np
import pytest
import torch

import eval_oracle as eo
from conftest import load_golden
from vmap_amd import _lib, evaluation, meshing

CLOUDS = ("uniform", "clustered", "duplicates", "room5m")


@pytest.mark.parametrize("name", CLOUDS)
def test_oracle_equals_ckdtree_fixtures(name):
    g = load_golden(f"eval_{name}")
    for q, r, d_ref, i_ref in ((g["rec"], g["gt"], g["d_rec_gt"], g["i_rec_gt"]), (g["gt"], g["rec"], g["d_gt_rec"], g["i_gt_rec"])):
        d, i = eo.nn(q, r)
        np.testing.assert_allclose(d, d_ref, rtol=0, atol=1e-12)
        # indices: equal wherever the nearest ref is unique (cKDTree does not promise the smallest index among exact ties)
        r64 = np.asarray(r, np.float64)
        unique = ~np.array([np.sum(np.all(r64 == r64[j], axis=1)) > 1 for j in i]) & (eo.runner_up_gap(q, r) > 0)
        assert unique.sum() > len(q) // 4
        np.testing.assert_array_equal(i[unique], i_ref[unique])
    m = eo.metrics(g["gt"], g["rec"])
    np.testing.assert_allclose([x[0] for x in m], g["metrics"], rtol=1e-12, atol=0)
    assert abs(eo.chamfer(g["gt"], g["rec"]) - (g["metrics"][0] + g["metrics"][1]) / 2) < 1e-12


def test_oracle_equals_ckdtree_live():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(5)
    q, r = rng.normal(size=(700, 3)), rng.normal(size=(900, 3)) * 1.2 + 0.1
    d, i = eo.nn(q, r, chunk=97)
    dk, ik = spatial.cKDTree(r).query(q)
    np.testing.assert_allclose(d, dk, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(i, ik)


def test_oracle_ties_go_to_the_smallest_index():
    r = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0]], np.float64)
    d, i = eo.nn(np.zeros((1, 3)), r)
    assert d[0] == 1.0 and i[0] == 0


def test_clip_unit_cube_keeps_the_exact_area():
    # the unit cube [0,1]^3 as 12 triangles, cut by an axis-aligned box [0.25, 2] x [-1, 0.5] x [0.1, 0.9]
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    lo, hi = np.array([0.25, -1.0, 0.1]), np.array([2.0, 0.5, 0.9])
    tris = eo.clip_mesh(v, f, (lo + hi) / 2, np.eye(3), hi - lo)
    # what lies inside: the x=1 face (0.5 x 0.8) and the y=0 face (0.75 x 0.8); the faces x=0, y=1, z=0 and z=1 lie outside
    dx, dy, dz = 0.75, 0.5, 0.8
    want = dy * dz + dx * dz
    assert abs(eo.soup_area(tris) - want) < 1e-12
    assert np.all(tris >= lo - 1e-12) and np.all(tris <= hi + 1e-12)


def test_clip_tetrahedron_half_inside_and_a_rotated_box():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    # half-space x <= 0.5 as a huge box: the part of the tetrahedron's surface with x <= 0.5
    tris = eo.clip_mesh(v, f, [0.5 - 50, 0, 0], np.eye(3), [100, 100, 100])
    # faces z=0 and y=0: the right triangle legs 1 minus the corner x > 0.5 (area 1/8); face x=0: 1/2 whole; slanted face
    # (area sqrt(3)/2) minus its corner x > 0.5 (scale 1/2 -> a quarter)
    want = 2 * (0.5 - 0.125) + 0.5 + np.sqrt(3) / 2 * 0.75
    assert abs(eo.soup_area(tris) - want) < 1e-12
    # the same cut through a rotated frame: rotate the mesh and the box together, the area is unchanged
    th = 0.7
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    tris2 = eo.clip_mesh(v @ Rz.T, f, Rz @ np.array([0.5 - 50, 0, 0]), Rz, [100, 100, 100])
    assert abs(eo.soup_area(tris2) - want) < 1e-12
    # a triangle inside is kept as it is
    inside = eo.clip_mesh(v, f[:1], [0, 0, 0], np.eye(3), [10, 10, 10])
    np.testing.assert_array_equal(inside[0], v[f[0]])


def test_sampling_formula():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2], [1, 0, 2], [0, 3, 2]], np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5]])          # areas 0.5 and 1.5
    pts, face = eo.sample(v, f, [0.1, 0.3, 0.9], [[0.2, 0.3], [0.9, 0.8], [0.5, 0.25]])
    np.testing.assert_array_equal(face, [0, 1, 1])
    np.testing.assert_allclose(pts[0], [0.2, 0.3, 0])
    np.testing.assert_allclose(pts[1], [0.1, 3 * 0.2, 2])            # r1 + r2 > 1: folded to (0.1, 0.2)


def _write_ply_binary(path, verts, faces, vdtype="<f8", extra=True, count_type="u1", index_type="<i4"):
    vprops = [("x", vdtype), ("y", vdtype), ("z", vdtype)]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(verts)}"]
    tmap = {"<f8": "double", "<f4": "float", "u1": "uchar", "<i4": "int", "<u4": "uint", "<i2": "short"}
    head += [f"property {tmap[t]} {n}" for n, t in vprops]
    if extra:
        head += ["property uchar red", "property uchar green", "property uchar blue", "property short object_id"]
        vprops += [("r", "u1"), ("g", "u1"), ("b", "u1"), ("oid", "<i2")]
    head += [f"element face {len(faces)}", f"property list {tmap[count_type]} {tmap[index_type]} vertex_indices"]
    if extra:
        head += ["property int object_id"]
    head += ["end_header"]
    vert = np.zeros(len(verts), dtype=vprops)
    vert["x"], vert["y"], vert["z"] = verts[:, 0], verts[:, 1], verts[:, 2]
    body = bytearray(vert.tobytes())
    for poly in faces:
        body += np.array([len(poly)], count_type).tobytes() + np.array(poly, index_type).tobytes()
        if extra:
            body += np.array([7], "<i4").tobytes()
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(bytes(body))


def test_load_mesh_reads_binary_and_ascii_ply_with_quads_and_extra_properties(tmp_path):
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.0 / 3.0]], np.float64)
    polys = [[0, 1, 2, 3], [0, 1, 4], [1, 2, 4]]
    want = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4]])
    for i, kw in enumerate([dict(), dict(vdtype="<f4", extra=False), dict(count_type="<i4", index_type="<u4")]):
        p = tmp_path / f"b{i}.ply"
        _write_ply_binary(p, verts, polys, **kw)
        m = meshing.load_mesh(p, device="cpu")
        np.testing.assert_array_equal(m.vertices.numpy(), verts.astype(np.float32))
        np.testing.assert_array_equal(m.faces.numpy(), want)
        assert m.vertex_normals is None and m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32
    p = tmp_path / "a.ply"
    p.write_text("ply\nformat ascii 1.0\ncomment handmade\nelement vertex 5\nproperty double x\nproperty double y\nproperty double z\n"
                 "property uchar red\nelement face 3\nproperty list uchar int vertex_indices\nproperty int object_id\nend_header\n"
                 + "".join(f"{float(x)!r} {float(y)!r} {float(z)!r} 200\n" for x, y, z in verts)
                 + "".join(f"{len(q)} {' '.join(map(str, q))} 3\n" for q in polys))
    m = meshing.load_mesh(p, device="cpu")
    np.testing.assert_array_equal(m.vertices.numpy(), verts.astype(np.float32))
    np.testing.assert_array_equal(m.faces.numpy(), want)


@pytest.mark.parametrize("ext", ["obj", "ply"])
@pytest.mark.parametrize("normals", [True, False])
def test_load_mesh_round_trips_export(tmp_path, ext, normals):
    rng = np.random.default_rng(3)
    v = torch.from_numpy(rng.normal(size=(40, 3)).astype(np.float32))
    f = torch.from_numpy(rng.integers(0, 40, (60, 3)).astype(np.int32))
    n = torch.from_numpy(rng.normal(size=(40, 3)).astype(np.float32)) if normals else None
    c = torch.from_numpy(rng.integers(0, 256, (40, 3)).astype(np.uint8))
    p = tmp_path / f"m.{ext}"
    meshing.Mesh(v, f, n, c).export(p)
    m = meshing.load_mesh(p, device="cpu")
    np.testing.assert_array_equal(m.faces.numpy(), f.numpy())
    if ext == "ply":
        np.testing.assert_array_equal(m.vertices.numpy(), v.numpy())
    else:
        np.testing.assert_allclose(m.vertices.numpy(), v.numpy(), rtol=1e-6, atol=1e-7)


def test_load_mesh_obj_polygons_and_slashes(tmp_path):
    p = tmp_path / "q.obj"
    p.write_text("# quad\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1 4/1/1\nf -4 -3 -1\n")
    m = meshing.load_mesh(p, device="cpu")
    np.testing.assert_array_equal(m.faces.numpy(), [[0, 1, 2], [0, 2, 3], [0, 1, 3]])


def test_principal_axes_box_of_a_rotated_box_cloud():
    rng = np.random.default_rng(11)
    ext = np.array([3.0, 1.6, 0.5])
    # a regular grid over the box (its covariance is diagonal in the box's frame), shuffled
    g = np.linspace(-0.5, 0.5, 11)
    local = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(11 ** 3)] * ext
    a, b = 0.4, -0.9
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R = Rz @ Rx
    c = np.array([4.0, -2.0, 1.0])
    box = evaluation.principal_axes_box(local @ R.T + c)
    assert np.linalg.det(box.R) > 0.999
    np.testing.assert_allclose(np.abs(box.R.T @ R), np.eye(3), atol=1e-9)       # the same axes up to sign, in extent order
    np.testing.assert_allclose(box.extent, ext, atol=1e-9)
    np.testing.assert_allclose(box.center, c, atol=1e-9)


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_eval_abi_argument_checks():
    lib = _lib.load()
    nb = ctypes.c_size_t()
    assert lib.vmapstep_nn_workspace_bytes(1000, 3, ctypes.byref(nb)) == 0 and nb.value >= 8000 and nb.value % 256 == 0
    assert lib.vmapstep_nn_workspace_bytes(1000, 3, None) == -1
    assert lib.vmapstep_nn_workspace_bytes(-1, 3, ctypes.byref(nb)) == -1
    assert lib.vmapstep_nn_workspace_bytes(1 << 31, 3, ctypes.byref(nb)) == -1
    p = ctypes.c_void_p(256 * 7)             # never dereferenced: every call below fails its checks first
    assert lib.vmapstep_nn_workspace_bytes(10, 2, ctypes.byref(nb)) == 0
    ws = nb.value

    def nn(qo, ro, nq=10, nr=10, n_sets=2, q=p, r=p, dist=p, w=p, wb=ws):
        return lib.vmapstep_nn_distance(q, nq, p, qo, r, nr, p, ro, n_sets, dist, None, w, wb, None)
    assert nn(None, _i64(0, 5, 10)) == -1                               # host offsets missing
    assert nn(_i64(0, 5, 10), None) == -1
    assert nn(_i64(0, 6, 5), _i64(0, 5, 10)) == -1                      # not monotone
    assert b"decrease" in lib.vmapstep_last_error()
    assert nn(_i64(-1, 5, 10), _i64(0, 5, 10)) == -1                    # below 0
    assert nn(_i64(0, 5, 11), _i64(0, 5, 10)) == -1                     # past the query array
    assert b"past" in lib.vmapstep_last_error()
    assert nn(_i64(0, 5, 10), _i64(0, 5, 12)) == -1                     # past the ref array
    assert nn(_i64(0, 5, 10), _i64(0, 5, 5)) == -1                      # set 1 has queries and no refs
    assert b"no refs" in lib.vmapstep_last_error()
    assert nn(_i64(0, 5, 10), _i64(0, 5, 10), n_sets=0) == -1
    assert nn(_i64(0, 5, 10), _i64(0, 5, 10), q=None) == -1             # null device arrays
    assert nn(_i64(0, 5, 10), _i64(0, 5, 10), dist=None) == -1
    assert nn(_i64(0, 5, 10), _i64(0, 5, 10), nq=1 << 31) == -1
    assert nn(_i64(0, 5, 10), _i64(0, 5, 10), w=None) == -3
    assert nn(_i64(0, 5, 10), _i64(0, 5, 10), wb=ws - 1) == -3
    assert nn(_i64(0, 5, 10), _i64(0, 5, 10), w=ctypes.c_void_p(256 * 7 + 8)) == -3
    # no query in any set: nothing to write, accepted without touching the device (an empty query set may have no refs)
    assert nn(_i64(3, 3, 3), _i64(0, 0, 4), q=None, r=None, dist=None, w=None) == 0

    assert lib.vmapstep_surface_sample_workspace_bytes(100, ctypes.byref(nb)) == 0 and nb.value >= 800 and nb.value % 256 == 0
    assert lib.vmapstep_surface_sample_workspace_bytes(-1, ctypes.byref(nb)) == -1
    sws = nb.value

    def ss(fo, oo, n_sets=2, nv=30, nf=100, randoms=None, out=p, w=p, wb=sws):
        return lib.vmapstep_surface_sample(p, nv, p, nf, p, fo, p, oo, n_sets, 0, 0, 0, randoms, out, None, w, wb, None)
    assert ss(None, _i64(0, 5, 10)) == -1
    assert ss(_i64(0, 50, 100), None) == -1
    assert ss(_i64(0, 60, 50), _i64(0, 5, 10)) == -1
    assert ss(_i64(0, 50, 101), _i64(0, 5, 10)) == -1                   # past the faces
    assert ss(_i64(0, 50, 100), _i64(0, 5, 4)) == -1
    assert ss(_i64(0, 100, 100), _i64(0, 5, 10)) == -1                  # set 1 has points and no faces
    assert b"no faces" in lib.vmapstep_last_error()
    assert ss(_i64(0, 50, 100), _i64(0, 5, 10), nv=-1) == -1
    half = _lib.SurfaceRandoms(256, None)
    assert ss(_i64(0, 50, 100), _i64(0, 5, 10), randoms=ctypes.byref(half)) == -1
    assert ss(_i64(0, 50, 100), _i64(0, 5, 10), out=None) == -1
    assert ss(_i64(0, 50, 100), _i64(0, 5, 10), wb=sws - 1) == -3
    assert ss(_i64(0, 100, 100), _i64(0, 0, 0), out=None, w=None) == 0  # no points: nothing to do

    assert lib.vmapstep_clip_box_workspace_bytes(1000, ctypes.byref(nb)) == 0 and nb.value >= 8 * 4 and nb.value % 256 == 0
    assert lib.vmapstep_clip_box_workspace_bytes(-5, ctypes.byref(nb)) == -1
    cws = nb.value
    box = (ctypes.c_float * 15)(0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1)
    bad = (ctypes.c_float * 15)(0, 0, float("nan"), 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1)
    assert lib.vmapstep_clip_box_count(None, 30, p, 1000, box, p, p, cws, None) == -1
    assert lib.vmapstep_clip_box_count(p, 30, None, 1000, box, p, p, cws, None) == -1
    assert lib.vmapstep_clip_box_count(p, 30, p, 1000, None, p, p, cws, None) == -1
    assert lib.vmapstep_clip_box_count(p, 30, p, 1000, bad, p, p, cws, None) == -1
    assert lib.vmapstep_clip_box_count(p, 30, p, 1000, box, None, p, cws, None) == -1
    assert lib.vmapstep_clip_box_count(p, 30, p, -1, box, p, p, cws, None) == -1
    assert lib.vmapstep_clip_box_count(p, 30, p, 1000, box, p, p, cws - 1, None) == -3
    assert lib.vmapstep_clip_box_emit(p, 30, p, 1000, box, None, 10, p, cws, None) == -1
    assert lib.vmapstep_clip_box_emit(p, 30, p, 1000, box, p, -1, p, cws, None) == -1
    assert lib.vmapstep_clip_box_emit(p, 30, p, 1000, box, p, 10, None, cws, None) == -3
    assert lib.vmapstep_clip_box_emit(p, 30, p, 1000, box, None, 0, p, cws, None) == 0


def test_surface_randoms_struct_matches_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmapstep.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(vmapstep_surface_randoms), offsetof(vmapstep_surface_randoms, r));\n  return 0;\n}\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(_lib.SurfaceRandoms) and off == _lib.SurfaceRandoms.r.offset


def test_evaluation_has_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.VmapStepError):
        evaluation.nn_distance(np.zeros((4, 3)), np.zeros((4, 3)))
