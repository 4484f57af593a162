"""CPU tier of the mesh rasteriser: csrc/raster_rules.h - compiled into the host program tests/tools/raster_rules_host.cpp with the
address and undefined-behaviour sanitizers - against the exact layer of the numpy checker (tests/raster_oracle.py) bit for bit, that
layer against the float64 geometry outside the ambiguous pixels, the deliberate cases of the contract with their answers written
out, and the argument checks of the raster entries of the C ABI (no device is touched).  Nothing is held against an outside
implementation: the contract of include/vmapstep.h is this project's own."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import raster_cases as rc
import raster_oracle as ro
from conftest import ROOT
from vmap_amd import _lib

f32 = np.float32


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """A stand-alone program with its own main, built with -fsanitize=address,undefined: any out-of-bounds access or undefined
    arithmetic in the rules aborts it."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("raster_host") / "raster_rules_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vmap_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "raster_rules_host.cpp"), "-o", exe], check=True)
    return exe


def hexes(a):
    return " ".join(f"{x:08x}" for x in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32).tolist())


def run_host(exe, tmp_path, vertices, faces, t_wc, intrinsics, width, height, min_depth, max_depth=0.0):
    t_wc = np.asarray(t_wc, np.float32).reshape(-1, 4, 4)
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lines = [hexes(list(intrinsics) + [min_depth, max_depth]), f"{width} {height} {len(t_wc)} {len(vertices)} {len(faces)}", hexes(t_wc[:, :3, :]),
             hexes(vertices), " ".join(str(int(i)) for i in faces.reshape(-1))]
    path = tmp_path / "scene.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, "raster", str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    K, pixels = len(t_wc), width * height
    dropped = np.zeros(K, np.int64)
    depth, face, covered = np.zeros((K, pixels), np.uint32), np.zeros((K, pixels), np.int32), np.zeros((K, pixels), np.int32)
    for k in range(K):
        head = out[k * (pixels + 1)].split()
        assert head[:2] == ["view", str(k)]
        dropped[k] = int(head[3])
        rows = [l.split() for l in out[k * (pixels + 1) + 1:(k + 1) * (pixels + 1)]]
        depth[k] = [int(r[0], 16) for r in rows]
        face[k] = [int(r[1]) for r in rows]
        covered[k] = [int(r[2]) for r in rows]
    shape = (K, width, height)
    return dict(depth=depth.view(np.float32).reshape(shape), face=face.reshape(shape), dropped=dropped, covered=covered.reshape(shape))


def same(a, b, keys=("depth", "face", "dropped", "covered")):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), np.asarray(y, np.float32).view(np.uint32)
        assert np.array_equal(x, y), k


SCENES = [(37, 23, 300, 3, 0.05, 0.0), (64, 48, 400, 2, 0.1, 3.5)]


@pytest.mark.parametrize("width,height,n,K,min_depth,max_depth", SCENES)
def test_host_program_equals_the_exact_checker(host_exe, tmp_path, width, height, n, K, min_depth, max_depth):
    """Random triangle soups with a NaN vertex, indices out of range, a face behind the camera, a face outside the guard band and an
    all-zero pose: depth, face, dropped and the coverage count, bit for bit."""
    v, f, t_wc, intr = rc.random_scene(width, height, n, K, seed=width + K)
    want = ro.raster_f32(v, f, t_wc, intr, width, height, min_depth, max_depth)
    got = run_host(host_exe, tmp_path, v, f, t_wc, intr, width, height, min_depth, max_depth)
    same(got, want)
    assert (want["dropped"][:K] >= 5).all() and (want["dropped"][:K] < n // 2).all() and want["dropped"][K] == n       # the spare pose drops all
    assert not (want["face"][K] >= 0).any() and 0.2 < (want["face"][:K] >= 0).mean() < 0.98
    assert not np.isin(want["face"], [0, 1, 2]).any()                                 # the NaN face and the two with bad indices
    assert not np.isin(want["face"][0], [3, 4]).any()                                 # behind camera 0 / outside its guard band
    assert want["covered"].max() >= 3                                                 # faces overlap: the z-buffer decides something
    if max_depth > 0:
        assert want["depth"].max() <= max_depth
        assert (ro.raster_f32(v, f, t_wc, intr, width, height, min_depth)["depth"] > max_depth).any()


def test_exact_checker_agrees_with_the_geometry_outside_the_ambiguous_pixels():
    """The coarse sphere-over-plane scene.  Outside the pixels whose centre lies within BAND = 1/64 pixel of a projected edge, hit
    and miss are equal and the depth differs by at most z^2 (|g_u| + |g_v|) / 256 + 1e-5 z.  Derived, not measured: snapping moves a
    corner by at most 1/512 pixel per axis, so the face's reciprocal-depth plane r(u, v) - affine in the image - moves by at most
    (|g_u| + |g_v|) / 512 at any pixel; dz = z^2 dr; the bound allows twice that, plus float32 rounding of the projection (1e-5 z)."""
    v, f, t_wc = rc.sphere_plane_scene()
    W, H = rc.GEO_W, rc.GEO_H
    got = ro.raster_f32(v, f, t_wc, rc.GEO_INTRINSICS, W, H, rc.GEO_MIN_DEPTH)
    geo = ro.raster_f64(v, f, t_wc[0], rc.GEO_INTRINSICS, W, H, rc.GEO_MIN_DEPTH)
    amb = geo["ambiguous"]
    print(f"ambiguous pixels: {amb.sum()} of {amb.size} ({amb.mean():.4%})")
    assert amb.mean() <= 0.05
    hit = got["face"][0] >= 0
    assert np.array_equal(hit[~amb], geo["hit"][~amb])
    assert got["dropped"][0] == 0 and 0.5 < hit.mean() < 1.0
    both = hit & geo["hit"] & ~amb
    assert np.array_equal(got["face"][0][both], geo["face"][both])
    z = geo["depth"]
    bound = z * z * (np.abs(geo["g_u"]) + np.abs(geo["g_v"])) / 256 + 1e-5 * z
    err = np.abs(got["depth"][0].astype(np.float64) - z)
    print(f"worst depth error / bound: {(err[both] / bound[both]).max():.3f}")
    assert (err[both] <= bound[both]).all()
    assert len(np.unique(got["face"][0][hit])) > 60                                   # sphere and plane faces both win pixels


# ---- the deliberate cases: identity pose, fx = fy = 10, cx = cy = 0, z = 1: (0.1 i, 0.1 j, 1) projects onto the pixel centre (i, j) ----

def lattice(host_exe, tmp_path, v, f, min_depth=0.05, max_depth=0.0, t_wc=rc.IDENT):
    want = ro.raster_f32(v, f, t_wc, rc.LAT_INTRINSICS, rc.LAT_W, rc.LAT_H, min_depth, max_depth)
    same(run_host(host_exe, tmp_path, v, f, t_wc, rc.LAT_INTRINSICS, rc.LAT_W, rc.LAT_H, min_depth, max_depth), want)
    return want


def test_every_centre_of_the_lattice_is_covered_exactly_once(host_exe, tmp_path):
    """Every vertex, every cell edge and every diagonal of the lattice passes through pixel centres.  The tie rule gives such a centre
    to exactly one face, and the covered block is half-open: of the rectangle [2, 8] x [2, 6] of centres, those with 2 < w <= 8 and
    2 <= h < 6 (an edge pointing towards +h, or along +w, owns its ties)."""
    v, f = rc.lattice_scene()
    got = lattice(host_exe, tmp_path, v, f)
    want = np.zeros((rc.LAT_W, rc.LAT_H), np.int32)
    want[3:9, 2:6] = 1
    assert np.array_equal(got["covered"][0], want)
    assert np.array_equal(got["face"][0] >= 0, want == 1) and got["dropped"][0] == 0
    assert np.array_equal(got["depth"][0][want == 1].view(np.uint32), np.full(24, f32(1.0).view(np.uint32)))


def test_coincident_faces_zero_area_windings_and_depth_bounds(host_exe, tmp_path):
    sq = np.array([[0.2, 0.2, 1.0], [0.8, 0.2, 1.0], [0.8, 0.6, 1.0], [0.2, 0.6, 1.0], [0.5, 0.4, 1.0]], np.float32)
    # two coincident faces: the smaller index wins; the order of the list does not matter
    got = lattice(host_exe, tmp_path, sq, [[0, 1, 2], [0, 1, 2]])
    assert set(np.unique(got["face"][0])) == {-1, 0} and got["covered"][0].max() == 2
    # a zero-area face (a repeated vertex, and three corners in a line) covers nothing and is not dropped
    got = lattice(host_exe, tmp_path, sq, [[0, 1, 1], [0, 4, 2]])
    assert not (got["face"][0] >= 0).any() and got["covered"][0].max() == 0 and got["dropped"][0] == 0
    # both windings give the same image, bit for bit (depths slanted so that the interpolation has something to do)
    slant = sq.copy()
    slant[:, 2] = [1.0, 1.5, 2.25, 1.25, 2.0]
    slant[:, :2] *= slant[:, 2:3]                                                     # the projections stay where they were
    a = lattice(host_exe, tmp_path, slant, [[0, 1, 2]])
    b = lattice(host_exe, tmp_path, slant, [[0, 2, 1]])
    same(a, b)
    assert (a["face"][0] >= 0).sum() >= 3 and len(np.unique(a["depth"][0])) > 3
    # the max_depth cut: the far face is covered but not written; 0 means no bound
    far = sq.copy()
    far[:, 2] = 3.0
    far[:, :2] *= 3.0
    both = np.concatenate([sq[:4], far[:4]])
    faces = [[0, 1, 3], [4, 5, 6], [4, 6, 7]]
    cut = lattice(host_exe, tmp_path, both, faces, max_depth=2.0)
    free = lattice(host_exe, tmp_path, both, faces)
    assert set(np.unique(cut["face"][0])) == {-1, 0} and set(np.unique(free["face"][0])) == {-1, 0, 1, 2}
    assert np.array_equal(cut["covered"], free["covered"])
    at3 = lattice(host_exe, tmp_path, both, faces, max_depth=3.0)                      # z == max_depth is written
    same(at3, free)
    # a corner exactly at min_depth is dropped; one ulp beyond it takes part
    got = lattice(host_exe, tmp_path, sq, [[0, 1, 2]], min_depth=1.0)
    assert got["dropped"][0] == 1 and not (got["face"][0] >= 0).any()
    got = lattice(host_exe, tmp_path, sq, [[0, 1, 2]], min_depth=float(np.nextafter(f32(1.0), f32(0.0))))
    assert got["dropped"][0] == 0 and (got["face"][0] >= 0).any()
    # an all-zero pose: z = 0, everything dropped
    got = lattice(host_exe, tmp_path, sq, [[0, 1, 2], [0, 2, 3]], t_wc=np.zeros((1, 4, 4), np.float32))
    assert got["dropped"][0] == 2 and not (got["face"][0] >= 0).any()


def test_compare_rule(host_exe, tmp_path):
    """0 against a measurement, NaN, negative, equal depths, a rounded difference, infinities - the host program and the integer
    checker, with the answers written out."""
    nan, inf = float("nan"), float("inf")
    up = float(np.nextafter(f32(1.0), f32(2.0)))
    cases = [((1.0, 1.0), (0, 0)), ((0.0, 2.0), (2, 0)), ((2.0, 0.0), (1, 0)), ((0.0, 0.0), (3, 0)), ((nan, 1.0), (2, 0)), ((1.0, nan), (1, 0)),
             ((nan, nan), (3, 0)), ((-1.0, 1.0), (2, 0)), ((1.5, 1.0), (0, 1 << 19)), ((1.0, 1.5), (0, 1 << 19)), ((1.0, up), (0, 0)),
             ((1.0, 1.0 + 2.0 ** -20), (0, 1)), ((1.0, 1.0 + 2.0 ** -21), (0, 0)), ((1.0, 1.0 + 3 * 2.0 ** -21), (0, 2)),      # ties go to even
             ((inf, 1.0), (0, 0)), ((inf, inf), (0, 0)), ((3e38, 1.0), (0, 1 << 40)), ((2.0e6, 1.0), (0, 1 << 40))]
    a = np.array([c[0][0] for c in cases], np.float32)
    b = np.array([c[0][1] for c in cases], np.float32)
    path = tmp_path / "pairs.txt"
    path.write_text(f"{len(cases)}\n" + hexes(np.stack([a, b], 1)) + "\n")
    out = subprocess.run([host_exe, "compare", str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = [tuple(int(x) for x in l.split()) for l in out[:len(cases)]]
    assert got == [c[1] for c in cases]
    counts = ro.compare_counts(a[None], b[None])[0]
    cls = np.array([c[1][0] for c in cases])
    assert counts.tolist() == [(cls == 0).sum(), (cls == 1).sum(), (cls == 2).sum(), sum(c[1][1] for c in cases)]
    one = ro.compare_counts(np.array([[1.5, 0.0, 2.0]]), np.array([[1.0, 1.0, 2.25]]))
    assert one.tolist() == [[2, 0, 1, (1 << 19) + (1 << 18)]] and ro.l1_of(one)[0] == 0.375
    assert np.isnan(ro.l1_of(np.array([[0, 3, 1, 0]]))[0])


# ---- the C ABI's argument checks ------------------------------------------------------------------------------------------------------

def _cfg(**kw):
    d = dict(fx=60.0, fy=60.0, cx=18.0, cy=11.0, min_depth=0.05, max_depth=0.0, width=37, height=23)
    d.update(kw)
    return _lib.RasterCfg(**d)


def test_abi_refuses_bad_arguments_before_anything_is_enqueued():
    """Every rejected argument of the raster section returns VMAPSTEP_ERR_ARGUMENT (-1) with a message, a short or misaligned workspace
    -3; none of the calls reads a pointer or touches a device."""
    lib = _lib.load()
    assert all(e in _lib.EXPORTS for e in ("vmapstep_raster_workspace_bytes", "vmapstep_raster_count", "vmapstep_raster_draw",
                                           "vmapstep_raster_resolve", "vmapstep_depth_compare"))
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    ref = ctypes.byref
    nws, nlarge = ctypes.c_size_t(), ctypes.c_size_t()
    size = lib.vmapstep_raster_workspace_bytes
    assert size(1000, 3, 50, ref(nws), ref(nlarge)) == 0 and nws.value >= 4 * 3 * 16 and nlarge.value >= 50 * (8 + 64)
    need, lneed = nws.value, nlarge.value
    assert size(1000, 3, 50, None, ref(nlarge)) == -1 and size(1000, 3, 50, ref(nws), None) == -1
    assert size(-1, 3, 50, ref(nws), ref(nlarge)) == -1 and size(1000, 0, 50, ref(nws), ref(nlarge)) == -1
    assert size(1000, 65536, 50, ref(nws), ref(nlarge)) == -1 and size(1000, 3, -1, ref(nws), ref(nlarge)) == -1
    assert size(1 << 31, 3, 50, ref(nws), ref(nlarge)) == -1

    def count(cfg, nv=100, nf=1000, k=3, vertices=p, faces=p, t_wc=p, keys=p, dropped=p, counts=p, ws=p, nb=need):
        return lib.vmapstep_raster_count(cfg, vertices, nv, faces, nf, t_wc, None, k, keys, dropped, counts, ws, nb, None)

    def draw(cfg, nv=100, nf=1000, k=3, vertices=p, faces=p, t_wc=p, keys=p, nl=10, npairs=40, large=p, cap=50, lb=lneed, ws=p, nb=need):
        return lib.vmapstep_raster_draw(cfg, vertices, nv, faces, nf, t_wc, None, k, keys, nl, npairs, large, cap, lb, ws, nb, None)

    bad = (dict(width=0), dict(height=0), dict(width=-3), dict(width=16385), dict(height=16385), dict(min_depth=0.0), dict(min_depth=-0.5),
           dict(min_depth=float("nan")), dict(min_depth=float("inf")), dict(max_depth=float("nan")), dict(fx=0.0), dict(fy=float("nan")),
           dict(cy=float("inf")))
    for kw in bad:
        for call in (count, draw):
            assert call(ref(_cfg(**kw))) == -1 and lib.vmapstep_last_error().startswith(b"raster"), kw
    ok = ref(_cfg())
    for call in (count, draw):
        assert call(None) == -1
        assert call(ok, nv=-1) == -1 and call(ok, nf=-1) == -1 and call(ok, nf=1 << 31) == -1 and call(ok, nv=0) == -1
        assert call(ok, k=0) == -1 and call(ok, k=65536) == -1
        assert call(ok, vertices=None) == -1 and call(ok, faces=None) == -1 and call(ok, t_wc=None) == -1 and call(ok, keys=None) == -1
        assert call(ok, nb=need - 1) == -3 and call(ok, ws=p + 8) == -3 and call(ok, ws=None) == -3 and b"raster workspace" in lib.vmapstep_last_error()
    assert count(ok, dropped=None) == -1 and count(ok, counts=None) == -1
    assert draw(ok, nl=-1) == -1 and draw(ok, npairs=-1) == -1 and draw(ok, cap=-1) == -1
    assert draw(ok, nl=51) == -1 and b"too small" in lib.vmapstep_last_error()        # a capacity below the count
    assert draw(ok, nl=0, npairs=5) == -1 and draw(ok, nl=3001, cap=4000) == -1        # more large faces than views x faces
    assert draw(ok, lb=lneed - 1) == -3 and draw(ok, large=None) == -3 and draw(ok, large=p + 8) == -3
    assert b"large-face" in lib.vmapstep_last_error()
    assert draw(ok, nl=0, npairs=0, large=None, cap=0, lb=0) == 0                      # nothing to draw: nothing enqueued

    resolve = lambda n=10, keys=p, depth=p, face=p, labels=None, nf=5, label=None, seen=None: \
        lib.vmapstep_raster_resolve(keys, n, depth, face, labels, nf, label, seen, None)
    assert resolve(n=-1) == -1 and resolve(nf=-1) == -1 and resolve(keys=None) == -1 and resolve(depth=None) == -1 and resolve(face=None) == -1
    assert resolve(label=p) == -1 and b"face_labels" in lib.vmapstep_last_error()
    assert resolve(n=0, keys=None, depth=None, face=None) == 0

    compare = lambda a=p, b=p, k=2, n=100, out=p: lib.vmapstep_depth_compare(a, b, k, n, out, None)
    assert compare(a=None) == -1 and compare(b=None) == -1 and compare(out=None) == -1
    assert compare(k=0) == -1 and compare(k=65536) == -1 and compare(n=0) == -1 and compare(n=1 << 31) == -1
    assert b"depth_compare" in lib.vmapstep_last_error()
    assert lib.vmapstep_abi_version() == 7


def test_raster_cfg_layout_matches_the_header(tmp_path):
    """The ctypes mirror of vmapstep_raster_cfg against include/vmapstep.h as gcc lays it out."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = [f for f, _ in _lib.RasterCfg._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmapstep.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(vmapstep_raster_cfg));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(vmapstep_raster_cfg, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: int(l.split()[1]) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert got["size"] == ctypes.sizeof(_lib.RasterCfg)
    for f in fields:
        assert got[f] == getattr(_lib.RasterCfg, f).offset, f


def test_python_layer_refuses_what_it_can_without_a_device():
    import torch
    import vmap_amd
    from vmap_amd import raster
    assert set(raster.__all__) == {"Raster", "rasterize", "visible_faces", "cull_mesh_faces", "cull_to_raster", "compare_depth", "depth_l1"}
    assert "raster" in vmap_amd.__all__
    if not torch.cuda.is_available():
        v, f = rc.box_room()
        with pytest.raises(_lib.VmapStepError):
            raster.rasterize((v, f), rc.IDENT, rc.LAT_INTRINSICS, 8, 8, min_depth=0.05)
        with pytest.raises(_lib.VmapStepError):
            raster.compare_depth(np.zeros((1, 4, 4), np.float32), np.zeros((1, 4, 4), np.float32))
