"""GPU tier of the mesh rasteriser (vmap_amd/raster.py; csrc/raster_kernels.h): depth, face, label and dropped equal the exact layer of
the numpy checker (tests/raster_oracle.py) bit for bit - a z-buffer of integer minima has no tolerance - whatever the chunking and
from run to run; the visible-face cull, the depth comparison, the hand-over to FrameIngest and the command line.  Sizes: face counts
one below, at and one above a block of the setup pass (256), 3 212 small faces (the lane path), twelve faces that fill the image (the
tile path) at image sizes that are and are not multiples of the 8 x 8 tile."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import cull_cases as cc
import raster_cases as rc
import raster_oracle as ro
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(r):
    return dict(depth=r.depth.cpu().numpy(), face=r.face.cpu().numpy(), dropped=r.dropped.cpu().numpy(),
                label=None if r.label is None else r.label.cpu().numpy())


def assert_equal(got, want):
    assert got["depth"].dtype == np.float32 and got["face"].dtype == np.int32
    assert np.array_equal(got["face"], want["face"])
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(got["dropped"], want["dropped"])


def draw_twice(mesh, t_wc, intr, W, H, **kw):
    """rasterize, run twice and compared byte for byte"""
    from vmap_amd import raster
    a, b = host(raster.rasterize(mesh, t_wc, intr, W, H, **kw)), host(raster.rasterize(mesh, t_wc, intr, W, H, **kw))
    assert_equal(a, b)
    return a


@pytest.mark.parametrize("width,height,n,K,min_depth,max_depth", [
    (37, 23, 300, 3, 0.05, None), (64, 48, 400, 1, 0.1, 3.5), (64, 48, 400, 5, 0.1, 3.5),
    (37, 23, rc.SETUP_WG - 1, 1, 0.05, None), (37, 23, rc.SETUP_WG, 3, 0.05, None), (64, 48, rc.SETUP_WG + 1, 5, 0.05, 4.0)])
def test_images_equal_the_exact_checker(width, height, n, K, min_depth, max_depth):
    """The random soups of the CPU tier (a NaN vertex, indices out of range, a face behind the camera, one outside the guard band, an
    all-zero pose), K views + the empty one; both draw paths take part."""
    v, f, t_wc, intr = rc.random_scene(width, height, n, K, seed=width + K)
    want = ro.raster_f32(v, f, t_wc, intr, width, height, min_depth, max_depth)
    got = draw_twice((v, f), t_wc, intr, width, height, min_depth=min_depth, max_depth=max_depth)
    assert_equal(got, want)
    assert got["label"] is None and (want["face"][:K] >= 0).mean() > 0.2 and want["dropped"][K] == n
    # the views in another order, through slots
    from vmap_amd import raster
    order = list(range(K, -1, -1))
    again = host(raster.rasterize((v, f), t_wc, intr, width, height, min_depth=min_depth, max_depth=max_depth, slots=order))
    assert_equal(again, {k: want[k][order] for k in ("depth", "face", "dropped")})


@pytest.fixture(scope="module")
def sphere():
    """The lewiner mesh of the golden sphere, in metres, from three poses at 96 x 72, and the checker's images (computed once)."""
    g = load_golden("mesh_sphere")
    v, f = (g["lewiner_vertices"] * np.float32(0.01)).astype(np.float32), g["lewiner_faces"].astype(np.int32)
    c = v.mean(0).astype(np.float64)
    t_wc = np.stack([cc.pose(np.eye(3), c + [0.0, 0.0, -0.3]), cc.pose(cc.rotation([0, 1, 0], 0.5), c + [-0.15, 0.02, -0.26]),
                     cc.pose(cc.rotation([1, 0, 0], -(np.pi / 2 + 0.2)), c + [0.0, -0.3, 0.06])])
    intr = (90.0, 95.0, 47.25, 35.5)
    want = ro.raster_f32(v, f, t_wc, intr, 96, 72, 0.05)
    return v, f, t_wc, intr, want


def test_small_faces_of_a_marching_cubes_mesh(sphere):
    v, f, t_wc, intr, want = sphere
    assert len(f) == 3212 and (want["dropped"] == 0).all() and ((want["face"] >= 0).mean((1, 2)) > 0.15).all()
    got = draw_twice((v, f), t_wc, intr, 96, 72, min_depth=0.05)
    assert_equal(got, want)


def test_chunked_views_equal_one_chunk(sphere):
    from vmap_amd import raster
    v, f, t_wc, intr, want = sphere
    poses = np.concatenate([t_wc, t_wc[::-1], t_wc[:1]])
    one = host(raster.rasterize((v, f), poses, intr, 96, 72, min_depth=0.05))
    for budget in (96 * 72 * 8, 2 * 96 * 72 * 8 + 5, 1):                              # one view, two views per chunk, a budget below one view
        many = host(raster.rasterize((v, f), poses, intr, 96, 72, min_depth=0.05, budget_bytes=budget))
        assert_equal(many, one)
    assert_equal({k: one[k][:3] for k in one if k != "label"}, want)


@pytest.mark.parametrize("width,height", [(200, 120), (37, 23), (64, 46)])
def test_faces_that_fill_the_image(width, height):
    """The twelve-face room from inside: every pixel is hit by a wall that spans the whole image and more - the tile path, with its
    image-border tiles where width or height is no multiple of 8.  The walls a view does not face are dropped (no near-plane clipping)."""
    v, f = rc.box_room()
    t_wc, intr = rc.room_poses(), rc.room_intrinsics(width, height)
    want = ro.raster_f32(v, f, t_wc, intr, width, height, 0.05)
    assert (want["face"] >= 0).all() and (want["dropped"] >= 6).all() and (want["dropped"] <= 10).all()
    assert all(len(np.unique(want["face"][k])) >= 2 for k in range(3))
    got = draw_twice((v, f), t_wc, intr, width, height, min_depth=0.05)
    assert_equal(got, want)


def test_large_faces_behind_several_rounds_of_the_block_scan():
    """2.1 M faces in three views are 24 585 block totals, three rounds and a part of the one workgroup's scan (8192 blocks per round:
    vr::kRasterScanWG x vr::kScanPer).  Nearly all faces name vertex 0 three times and draw nothing; the room's walls sit at the first
    face, on both sides of a round's boundary and at the last face, so every large face's place and first pair carry a prefix across rounds."""
    SCAN_ROUND = 1024 * 8 * rc.SETUP_WG
    rv, rf = rc.box_room()
    n = SCAN_ROUND + 2 * rc.SETUP_WG + 3
    faces = np.zeros((n, 3), np.int32)
    at = [0, 1, SCAN_ROUND - 1, SCAN_ROUND, SCAN_ROUND + 1, n - 2, n - 1]
    faces[at] = rf[[2, 3, 10, 11, 0, 1, 8]]                                           # the seven faces that win pixels in room_poses' views
    W, H = 64, 46
    t_wc, intr = rc.room_poses(), rc.room_intrinsics(W, H)
    want = ro.raster_f32(rv, faces, t_wc, intr, W, H, 0.05)
    small = ro.raster_f32(rv, rf, t_wc, intr, W, H, 0.05)
    assert (want["face"] >= 0).all() and np.array_equal(want["depth"], small["depth"])
    assert set(np.unique(want["face"])) == set(at)
    got = draw_twice((rv, faces), t_wc, intr, W, H, min_depth=0.05)
    assert_equal(got, want)


def test_labels_and_the_hand_over_to_frame_ingest():
    """rasterize(face_labels=) with labels from label_components of a two-component mesh (a wall and a sphere in front of it); the
    label image and the rasterised depth go into FrameIngest.put, and both components come out as instances."""
    from vmap_amd import components, ingest, keyframes, raster
    W, H = 96, 72
    sv, sf = rc.uv_sphere(8, 10, 0.5, (0.2, 0.0, 1.6))
    pv, pf = rc.grid_plane(7, 5, -2.0, 2.0, -1.5, 1.5, 2.5)
    v, f = np.concatenate([pv, sv]).astype(np.float32), np.concatenate([pf, sf + len(pv)]).astype(np.int32)
    labels, n = components.label_components(raster.Mesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), None))
    assert n == 2
    face_labels = labels[torch.from_numpy(f[:, 0]).long().to(DEV)] + 1                # instance ids 1 and 2; 0 is nobody's
    t_wc = rc.sphere_plane_scene()[2]
    r = raster.rasterize((v, f), t_wc, rc.GEO_INTRINSICS, W, H, min_depth=0.05, face_labels=face_labels)
    want = ro.raster_f32(v, f, t_wc, rc.GEO_INTRINSICS, W, H, 0.05)
    got = host(r)
    assert_equal(got, want)
    fl = face_labels.cpu().numpy()
    assert np.array_equal(got["label"], np.where(want["face"] >= 0, fl[np.maximum(want["face"], 0)], -1))
    assert set(np.unique(got["label"])) == {-1, 1, 2}
    store = keyframes.FrameStore(2, W, H, device=DEV)
    ing = ingest.FrameIngest(store, 1.0, 8.0, bbox_scale=0.2, min_box=4, max_ids=16)
    inst = torch.clamp(r.label[0], min=0).t().contiguous()                            # [H, W]; empty pixels -> id 0
    res = ing.put(torch.zeros((H, W, 3), dtype=torch.uint8), r.depth[0].t().contiguous(), inst, None, torch.from_numpy(t_wc[0]), 0)
    assert {1, 2} <= set(res.ids)
    assert np.array_equal(store.depth[res.slot].cpu().numpy().view(np.uint32), got["depth"][0].view(np.uint32))


# ---- culling by what won a pixel ------------------------------------------------------------------------------------------------------

def test_visible_faces_and_their_compaction(sphere):
    from vmap_amd import raster
    v, f, t_wc, intr, want = sphere
    seen_want = ro.visible_faces(want["face"], len(f))
    assert 0.2 < seen_want.mean() < 0.9                                               # the back of the sphere is hidden
    kw = dict(min_depth=0.05)
    seen = raster.visible_faces((v, f), t_wc, intr, 96, 72, **kw)
    assert seen.dtype == torch.uint8 and np.array_equal(seen.cpu().numpy(), seen_want)
    half = raster.visible_faces((v, f), t_wc, intr, 96, 72, slots=[0], **kw)
    assert np.array_equal(half.cpu().numpy(), ro.visible_faces(want["face"][:1], len(f))) and half.sum() < seen.sum()
    both = raster.visible_faces((v, f), t_wc, intr, 96, 72, slots=[1, 2], seen=half, **kw)
    assert both is half and np.array_equal(both.cpu().numpy(), seen_want)
    # the compaction against numpy, with normals riding along
    normals = np.random.default_rng(0).random(v.shape).astype(np.float32)
    mesh = raster.Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(normals))
    out = raster.cull_mesh_faces(mesh, seen)
    kf = f[seen_want != 0]
    kept = np.unique(kf)
    new = np.full(len(v), -1, np.int64)
    new[kept] = np.arange(len(kept))
    assert np.array_equal(out.faces.cpu().numpy(), new[kf]) and np.array_equal(out.vertices.cpu().numpy(), v[kept])
    assert np.array_equal(out.vertex_normals.cpu().numpy(), normals[kept])
    same = raster.cull_to_raster(mesh, t_wc, intr, 96, 72, **kw)
    assert np.array_equal(same.faces.cpu().numpy(), new[kf])
    assert raster.cull_mesh_faces(mesh, np.zeros(len(f), np.uint8)) is None


def test_a_face_whose_corners_miss_every_frustum_is_kept():
    """One triangle far larger than the view, its three corners outside the image, its middle filling it: the rasteriser keeps it,
    cull_to_views - which judges a face by its corners - drops it.  This is the limit the rasteriser lifts."""
    from vmap_amd import raster, visibility
    W, H, intr = 37, 23, (40.0, 40.0, 18.0, 11.0)
    v = np.array([[-20.0, -10.0, 3.0], [20.0, -10.0, 3.0], [0.0, 30.0, 3.0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    mesh = raster.Mesh(torch.from_numpy(v), torch.from_numpy(f), None)
    r = raster.rasterize(mesh, rc.IDENT, intr, W, H, min_depth=0.05)
    assert (r.face == 0).all() and (r.depth == 3.0).all() and int(r.dropped[0]) == 0
    kept = raster.cull_to_raster(mesh, rc.IDENT, intr, W, H, min_depth=0.05)
    assert kept is not None and len(kept.faces) == 1
    assert visibility.cull_to_views(mesh, r.depth, rc.IDENT, intr, 0.05) is None
    assert visibility.cull_to_views(mesh, None, rc.IDENT, intr, None, size=(W, H)) is None


# ---- the depth comparison -------------------------------------------------------------------------------------------------------------

def test_compare_depth_equals_the_integer_checker(sphere):
    from vmap_amd import raster
    rng = np.random.default_rng(4)
    K, W, H = 3, 67, 41                                                               # 2747 pixels: two blocks and a part of a third
    a = (1.0 + 2.0 * rng.random((K, W, H))).astype(np.float32)
    b = (a + (rng.random((K, W, H)) - 0.5).astype(np.float32) * np.float32(0.2)).astype(np.float32)
    a[rng.random(a.shape) < 0.2] = 0.0
    b[rng.random(b.shape) < 0.2] = 0.0
    a[0, 3, 4], b[0, 5, 6], a[1, 0, 0], b[1, 0, 0] = np.nan, np.nan, np.inf, 1.0
    a[2, 1, 1], b[2, 1, 1], a[2, 2, 2] = -1.0, 2.0, -0.0
    b[2] = 0.0                                                                        # a view without a single common pixel
    want = ro.compare_counts(a, b)
    got = raster.compare_depth(a, b)
    again = raster.compare_depth(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    for g in (got, again):
        assert np.array_equal(np.stack([g["n_both"], g["n_a_only"], g["n_b_only"], g["sum_q"]], 1), want)
        assert np.array_equal(g["l1"][:2], ro.l1_of(want)[:2]) and np.isnan(g["l1"][2])
    assert want[0, 0] > 1000 and want[2, 0] == 0 and 0.04 < got["l1"][0] < 0.06
    # depth_l1 of a mesh against itself is 0 over exactly the pixels that were hit; against a stack of depth images too
    v, f, t_wc, intr, ref = sphere
    d = raster.depth_l1((v, f), (v, f), t_wc, intr, 96, 72, min_depth=0.05)
    hits = (ref["face"] >= 0).sum((1, 2))
    assert np.array_equal(d["n_both"], hits) and not d["sum_q"].any() and not d["n_a_only"].any() and not d["n_b_only"].any() and d["depth_l1"] == 0.0
    shifted = np.where(ref["depth"] > 0, ref["depth"] + np.float32(0.25), 0).astype(np.float32)
    d = raster.depth_l1(shifted, (v, f), t_wc, intr, 96, 72, min_depth=0.05)
    assert np.array_equal(d["n_both"], hits) and abs(d["depth_l1"] - 0.25) < 1e-6


# ---- the command line -----------------------------------------------------------------------------------------------------------------

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
        code = evaluation.main(argv)
    return code, buf.getvalue()


def test_cli_renders_the_ground_truth_depth_and_reports_depth_l1(tmp_path, sphere):
    """python -m vmap_amd.evaluation REC GT --frames F --render-gt-depth --depth-l1 with a frames file that holds no depth: the JSON
    gains depth_l1, depth_both_share and depth_gt_only_share, and both meshes are culled.  The same command without the new flags and
    with a depth array prints exactly the keys it printed before the flags existed."""
    from vmap_amd import meshing, raster
    g = load_golden("mesh_sphere")
    v, f, t_wc, intr, want = sphere
    rec, gt = str(tmp_path / "rec.obj"), str(tmp_path / "gt.obj")
    lv = g["lorensen_vertices"] * np.float32(0.01)
    _write_obj(rec, lv.mean(0) + (lv - lv.mean(0)) * np.float32(1.02), g["lorensen_faces"])       # the other triangulation, 2 mm too large
    _write_obj(gt, v, f)
    frames, frames_d = str(tmp_path / "poses.npz"), str(tmp_path / "frames.npz")
    np.savez(frames, t_wc=t_wc, intrinsics=np.array(intr, np.float32), size=np.array([96, 72]))
    np.savez(frames_d, t_wc=t_wc, intrinsics=np.array(intr, np.float32), depth=want["depth"])
    code, out = _run_cli([rec, gt, "--n", "3000", "--seed", "5", "--frames", frames, "--render-gt-depth", "--depth-l1", "--occlusion-eps", "0.05"])
    res = json.loads(out)
    assert code == 0 and res["gt_faces"] == int(ro.visible_faces(want["face"], len(f)).sum()) and 0 < res["rec_faces"] < len(g["lorensen_faces"])
    d = raster.depth_l1(meshing.load_mesh(rec), meshing.load_mesh(gt), t_wc, intr, 96, 72, min_depth=0.05)
    assert res["depth_l1"] == d["depth_l1"] and 0.0005 < res["depth_l1"] < 0.004
    assert res["depth_both_share"] == int(d["n_both"].sum()) / (3 * 96 * 72) and res["depth_both_share"] > 0.15
    assert res["depth_gt_only_share"] == int(d["n_b_only"].sum()) / (3 * 96 * 72) and res["depth_gt_only_share"] < 0.01
    code, out = _run_cli([rec, gt, "--n", "3000", "--seed", "5", "--frames", frames_d, "--occlusion-eps", "0.05"])
    assert code == 0 and list(json.loads(out)) == ["rec", "gt", "n", "seed", "accuracy", "completion", "completion_ratio_1cm", "completion_ratio_5cm",
                                                   "frames", "occlusion_eps", "rec_faces", "gt_faces"]
    code, out = _run_cli([rec, gt, "--n", "3000", "--seed", "5"])
    assert code == 0 and list(json.loads(out)) == ["rec", "gt", "n", "seed", "accuracy", "completion", "completion_ratio_1cm", "completion_ratio_5cm"]
