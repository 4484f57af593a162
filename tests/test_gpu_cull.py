"""GPU tier of visibility culling (vmap_amd/visibility.py; csrc/cull_kernels.h), through the C ABI and the Python API: the flags equal
the float32 layer of the numpy checker (tests/cull_oracle.py) exactly, the compaction equals plain numpy exactly - everything is a
set or an integer, there is no tolerance anywhere.  Sizes: one point up to one cull_mark tile + 1 (1025), one frame up to one LDS
chunk of frames + 1 (33), 255 .. 257 faces around one block of the compaction, and 70 000 faces, whose 274 block totals pass one
chunk of the block-total scan."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import cull_cases as cc
import cull_oracle as co
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE, CHUNK, BLOCK = 1024, 32, 256         # vc::kCullTile, vc::kFrameChunk, vc::kCullWG (csrc/launch_geometry.h)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("n,K,size,eps,margin,min_depth", [
    (1, 1, (37, 23), 0.02, 0, 0.0), (63, 2, (37, 23), 0.02, 0, 0.0), (64, CHUNK, (64, 48), 0.05, 3, 0.5), (65, CHUNK + 1, (37, 23), None, 0, 0.0),
    (257, 2, (64, 48), None, 5, 1.0), (TILE + 1, CHUNK + 1, (37, 23), 0.02, 2, 0.0), (TILE + 1, 1, (64, 48), 0.05, 0, 0.0),
    (2 * TILE + 65, 2 * CHUNK + 3, (37, 23), 0.05, 0, 0.25)])
def test_flags_equal_the_float32_checker(n, K, size, eps, margin, min_depth):
    from vmap_amd import visibility
    W, H = size
    pts, depth, t_wc, intr = cc.random_scene(W, H, n, K, seed=n + K)
    if n > 10:
        pts[5] = [np.nan, 0.1, 0.2]
    want = co.seen_f32(pts, depth, t_wc, intr, W, H, eps, margin, min_depth)
    got = visibility.mark_visible(pts, depth, t_wc, intr, eps, margin=margin, min_depth=min_depth)
    assert got.dtype == torch.uint8 and got.device == torch.device(DEV) and got.shape == (n,)
    assert np.array_equal(got.cpu().numpy(), want)
    if n > 200:
        assert 0.05 < want.mean() < 0.98


def test_slots_as_a_permutation_with_gaps_and_a_store_read_in_place():
    """Frame k reads slot slots[k]; the unused slots are all zero and see nothing; mark_visible_store defaults to the used slots."""
    from vmap_amd import keyframes, visibility
    W, H, n, K = 37, 23, 700, 5
    pts, depth, t_wc, intr = cc.random_scene(W, H, n, K, seed=3)
    slots = [6, 1, 9, 4, 0]
    store = keyframes.FrameStore(11, W, H, device=DEV)
    for k, s in enumerate(slots):
        store.depth[s], store.t_wc[s], store.frame_of_slot[s] = dev(depth[k]), dev(t_wc[k]), 100 + k
    want = co.seen_f32(pts, depth, t_wc, intr, W, H, 0.02)
    got = visibility.mark_visible(pts, store.depth, store.t_wc, intr, 0.02, slots=slots)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(visibility.mark_visible_store(pts, store, intr, 0.02).cpu().numpy(), want)
    two = co.seen_f32(pts, depth, t_wc, intr, W, H, 0.02, slots=[3, 1])
    assert np.array_equal(visibility.mark_visible_store(pts, store, intr, 0.02, slots=[4, 1]).cpu().numpy(), two) and two.sum() < want.sum()
    every = visibility.mark_visible(pts, store.depth, store.t_wc, intr, 0.02)          # all 11 slots: the empty ones add nothing
    assert np.array_equal(every.cpu().numpy(), want)
    from vmap_amd import _lib
    with pytest.raises(_lib.VmapStepError):
        visibility.mark_visible(pts, store.depth, store.t_wc, intr, 0.02, slots=[0, 11])


def test_accumulation_and_frustum_only():
    """A seen that is already 1 stays 1; frames marked in two calls equal one call; frustum only with depth=None."""
    from vmap_amd import visibility
    W, H, n, K = 64, 48, 1500, CHUNK + 5
    pts, depth, t_wc, intr = cc.random_scene(W, H, n, K, seed=8)
    one = visibility.mark_visible(pts, depth, t_wc, intr, 0.05)
    want = co.seen_f32(pts, depth, t_wc, intr, W, H, 0.05)
    assert np.array_equal(one.cpu().numpy(), want)
    first = visibility.mark_visible(pts, depth, t_wc, intr, 0.05, slots=range(0, 7))
    assert first.sum() < one.sum()
    both = visibility.mark_visible(pts, depth, t_wc, intr, 0.05, slots=range(7, K), seen=first)
    assert both is first and torch.equal(both, one)
    pre = np.zeros(n, np.uint8)
    pre[::3] = 1
    got = visibility.mark_visible(pts, depth, t_wc, intr, 0.05, seen=dev(pre))
    assert np.array_equal(got.cpu().numpy(), np.maximum(pre, want)) and (pre > want).any()
    frus = visibility.mark_visible(pts, None, t_wc, intr, None, size=(W, H))
    assert np.array_equal(frus.cpu().numpy(), co.seen_f32(pts, None, t_wc, intr, W, H, None)) and frus.sum() > one.sum()
    none = visibility.mark_visible(pts, depth, t_wc, intr, 0.05, slots=[])         # no frame: nothing written
    assert none.sum() == 0


def _compact_abi(faces, seen, min_seen):
    """vmapstep_cull_faces_count / _emit with outputs one element longer than the counts, poisoned: nothing at or past them is written."""
    from vmap_amd import _devmem, _lib
    lib = _lib.load()
    f, s = dev(faces.astype(np.int32)), dev(seen.astype(np.uint8))
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_cull_workspace_bytes, torch.device(DEV), len(seen), len(faces))
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    st = _devmem.stream(torch.device(DEV))
    _lib.check(lib.vmapstep_cull_faces_count(f.data_ptr(), len(f), s.data_ptr(), len(seen), min_seen, counts.data_ptr(), ws_ptr, nbytes, st), lib)
    nf, nv = counts.cpu().tolist()
    kept = torch.full((nv + 1,), -5, dtype=torch.int32, device=DEV)
    out = torch.full((nf + 1, 3), -5, dtype=torch.int32, device=DEV)
    _lib.check(lib.vmapstep_cull_faces_emit(f.data_ptr(), len(f), s.data_ptr(), len(seen), min_seen, kept.data_ptr(), nv, out.data_ptr(), nf,
                                            ws_ptr, nbytes, st), lib)
    kept, out = kept.cpu().numpy(), out.cpu().numpy()
    assert kept[nv] == -5 and (out[nf] == -5).all()
    return out[:nf], kept[:nv]


@pytest.mark.parametrize("F", [1, BLOCK - 1, BLOCK, BLOCK + 1, 70000])
@pytest.mark.parametrize("min_seen", [1, 2, 3])
def test_compaction_equals_numpy(F, min_seen):
    nv = F + 3
    rng = np.random.default_rng(F + min_seen)
    faces = cc.random_faces(nv, F, seed=F)
    for name, seen in (("random", (rng.random(nv) < 0.45).astype(np.uint8)), ("none", np.zeros(nv, np.uint8)), ("all", np.ones(nv, np.uint8))):
        want_f, want_k = co.cull_faces(faces, seen, min_seen)
        got_f, got_k = _compact_abi(faces, seen, min_seen)
        assert np.array_equal(got_k, want_k) and np.array_equal(got_f, want_f), name
        assert len(want_f) == {"none": 0, "all": F}.get(name, len(want_f))
    if F == 70000:
        assert -(-F // BLOCK) > 256 and -(-nv // BLOCK) > 256       # more blocks of faces and of vertices than one chunk of the block-total scan


def test_cull_mesh_carries_normals_and_colours_and_returns_none_when_nothing_is_left():
    from vmap_amd import meshing, visibility
    nv, F = 900, 1700
    rng = np.random.default_rng(4)
    faces = cc.random_faces(nv, F, seed=1)
    v = rng.standard_normal((nv, 3)).astype(np.float32)
    nrm = rng.standard_normal((nv, 3)).astype(np.float32)
    col = rng.integers(0, 256, (nv, 3)).astype(np.uint8)
    seen = (rng.random(nv) < 0.3).astype(np.uint8)
    mesh = meshing.Mesh(dev(v), dev(faces), dev(nrm), dev(col))
    for min_seen in (1, 2, 3):
        want_f, want_k = co.cull_faces(faces, seen, min_seen)
        got = visibility.cull_mesh(mesh, dev(seen), min_seen)
        assert np.array_equal(got.faces.cpu().numpy(), want_f) and got.faces.dtype == torch.int32
        assert np.array_equal(got.vertices.cpu().numpy(), v[want_k]) and np.array_equal(got.vertex_normals.cpu().numpy(), nrm[want_k])
        assert np.array_equal(got.vertex_colors.cpu().numpy(), col[want_k]) and got.vertex_colors.dtype == torch.uint8
    plain = visibility.cull_mesh(meshing.Mesh(dev(v), dev(faces), None), seen, 1)      # a host mask, no normals, no colours
    assert plain.vertex_normals is None and plain.vertex_colors is None and len(plain.faces) == len(co.cull_faces(faces, seen, 1)[0])
    assert visibility.cull_mesh(mesh, np.zeros(nv, np.uint8), 1) is None
    whole = visibility.cull_mesh(mesh, np.ones(nv, np.uint8), 3)         # every face stays; vertices no face names still go
    assert len(whole.faces) == F and torch.equal(whole.vertices[whole.faces.long()], mesh.vertices[mesh.faces.long()])


def test_known_answer_scene_on_the_device():
    """The wall and the box behind it: see tests/test_cull.py::test_known_answer_scene."""
    from vmap_amd import meshing, visibility
    s = cc.known_answer_scene()
    v, nw = s["vertices"], s["n_wall"]
    geo, amb = co.seen_f64(v, None, s["t_wc"], cc.KA_INTRINSICS, cc.KA_W, cc.KA_H, None)
    assert not amb.any()
    occl = visibility.mark_visible(v, s["depth"], s["t_wc"], cc.KA_INTRINSICS, cc.KA_EPS).cpu().numpy().astype(bool)
    frus = visibility.mark_visible(v, None, s["t_wc"], cc.KA_INTRINSICS, None, size=(cc.KA_W, cc.KA_H)).cpu().numpy().astype(bool)
    assert not occl[nw:].any() and frus[nw:].all()
    assert np.array_equal(occl[:nw], geo[:nw]) and np.array_equal(frus[:nw], geo[:nw]) and 10 < geo[:nw].sum() < nw - 100
    mesh = meshing.Mesh(dev(v), dev(s["faces"]), None)
    culled = visibility.cull_to_views(mesh, s["depth"], s["t_wc"], cc.KA_INTRINSICS, cc.KA_EPS)
    kept_z = culled.vertices[:, 2].cpu().numpy()
    assert len(culled.faces) > 0 and (kept_z == np.float32(cc.WALL_Z)).all()              # only wall faces are left
    both = visibility.cull_to_views(mesh, None, s["t_wc"], cc.KA_INTRINSICS, None, min_seen=3, size=(cc.KA_W, cc.KA_H))
    assert (both.vertices[:, 2] > cc.WALL_Z).sum() == 8                                   # frustum only: the box survives whole


def _write_obj(path, vertices, faces):
    with open(path, "w") as fh:
        for p in vertices:
            fh.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for f in faces:
            fh.write(f"f {f[0] + 1} {f[1] + 1} {f[2] + 1}\n")


def _run_cli(argv):
    from vmap_amd import evaluation
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = evaluation.main(argv)
    return rc, buf.getvalue()


def test_cli_culls_both_meshes_with_frames(tmp_path):
    """python -m vmap_amd.evaluation REC GT --frames FILE.npz --occlusion-eps X on two small generated files: the reconstruction is
    the wall and the box, the ground truth the wall alone; culled by the frames both are the seen part of the wall, and the
    result is calc_3d_metric's on the two culled meshes."""
    s = cc.known_answer_scene()
    nw = s["n_wall"]
    wall_faces = s["faces"][(s["faces"] < nw).all(1)]
    rec, gt, frames = tmp_path / "rec.obj", tmp_path / "gt.obj", tmp_path / "frames.npz"
    _write_obj(rec, s["vertices"], s["faces"])
    _write_obj(gt, s["vertices"][:nw], wall_faces)
    np.savez(frames, depth=s["depth"], t_wc=s["t_wc"], intrinsics=np.asarray(cc.KA_INTRINSICS, np.float32))
    rc, out = _run_cli([str(rec), str(gt), "--n", "2000", "--frames", str(frames), "--occlusion-eps", str(cc.KA_EPS)])
    assert rc == 0
    res = json.loads(out)
    assert res["rec_faces"] == res["gt_faces"] > 0 and res["occlusion_eps"] == cc.KA_EPS and res["frames"] == str(frames)
    assert res["gt_faces"] < len(wall_faces) and res["accuracy"] < 0.1 and res["completion"] < 0.1     # two samplings of one patch of the wall
    from vmap_amd import evaluation, meshing, visibility
    culled = [visibility.cull_to_views(meshing.load_mesh(str(m)), s["depth"], s["t_wc"], cc.KA_INTRINSICS, cc.KA_EPS) for m in (rec, gt)]
    m = evaluation.calc_3d_metric(culled[0], culled[1], N=2000, seed=0)
    assert [res["accuracy"], res["completion"], res["completion_ratio_1cm"], res["completion_ratio_5cm"]] == [x[0] for x in m]
    rc0, out0 = _run_cli([str(rec), str(gt), "--n", "2000"])
    assert rc0 == 0 and "frames" not in json.loads(out0) and "rec_faces" not in json.loads(out0)


def test_cli_output_without_the_flag_is_unchanged(tmp_path):
    """Without --frames the output is what calc_3d_metric gives, formatted as before the option existed - the same keys in the same
    order with the same values, byte for byte - on a golden mesh pair (tests/golden/mesh_sphere.npz: the two triangulations)."""
    from vmap_amd import evaluation, meshing
    g = load_golden("mesh_sphere")
    rec, gt = str(tmp_path / "rec.obj"), str(tmp_path / "gt.obj")
    _write_obj(rec, g["lewiner_vertices"] * np.float32(0.01), g["lewiner_faces"])
    _write_obj(gt, g["lorensen_vertices"] * np.float32(0.0102), g["lorensen_faces"])
    rc, out = _run_cli([rec, gt, "--n", "3000", "--seed", "5"])
    m = evaluation.calc_3d_metric(meshing.load_mesh(rec), meshing.load_mesh(gt), N=3000, seed=5)
    want = json.dumps({"rec": rec, "gt": gt, "n": 3000, "seed": 5, "accuracy": m[0][0], "completion": m[1][0],
                       "completion_ratio_1cm": m[2][0], "completion_ratio_5cm": m[3][0]}) + "\n"
    assert rc == 0 and out == want
