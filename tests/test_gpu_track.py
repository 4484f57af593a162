"""GPU tier of the instance tracker (vmap_amd/tracking.py; csrc/track_kernels.h): exact equality - the table of detection rows, the
inside count of every (row, candidate) pair, the sorted key set, the label image and the registry - with the numpy checker
(tests/track_oracle.py), which is handed the device's own float32 box table at every frame, so that the box search (covered by the
bounds tests) is out of the comparison.  Everything is integer or float32 with every rounding pinned: there is no tolerance anywhere.
The frames are tests/track_cases.py's: 75 x 53, a multiple of no tile dimension (two track_stats tiles across, four down; four blocks
of the linear kernels, the last one partial).  tests/test_track.py shows on the CPU that every case produces the status it is named
for."""
import numpy as np
import pytest
import torch

import ingest_oracle as io
import track_cases as tc
import track_oracle as to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_tracker(det_shift=0, **kw):
    from vmap_amd import tracking
    s = dict(tc.SETTINGS, **kw)
    return tracking.InstanceTracker(tc.W, tc.H, tc.INTRINSICS, s["depth_scale"], s["max_depth"], background_classes=s["background"],
                                    match_ratio=s["match_ratio"], min_pixels=s["min_pixels"], min_points=s["min_points"],
                                    erode_radius=s["erode_radius"], voxel_size=s["voxel_size"], min_extent=s["min_extent"], det_shift=det_shift,
                                    max_det=s["max_det"], max_pairs=s["max_pairs"], max_ids=s["max_ids"], device=DEV)


def make_oracle(det_shift=0, **kw):
    s = dict(tc.SETTINGS, **kw)
    return to.Tracker(tc.W, tc.H, tc.INTRINSICS, s["depth_scale"], s["max_depth"], s["background"], s["match_ratio"], s["min_pixels"], s["min_points"],
                      s["erode_radius"], s["voxel_size"], det_shift, s["max_det"], s["max_ids"])


def put_both(trk, orc, frame, wide=False):
    """One frame through the device and through the checker (with the box table the device judged it by); asserts equality of the
    rows, the pairs, the labels, the key state, the counters and the registry.  -> (TrackResult, oracle dict)"""
    rows, classes, depth, t_wc = frame
    d, det, _ = tc.typed(rows, depth, wide)
    table = trk.box_table.cpu().numpy().copy()
    res = trk.put(torch.from_numpy(d), torch.from_numpy(det), classes, t_wc)
    out = orc.put(d, det, classes, t_wc, table)
    assert res.rows.dtype == np.int32 and np.array_equal(res.rows, out["rows"]), (res.rows, out["rows"])
    assert np.array_equal(res.pairs, out["pairs"]), (res.pairs, out["pairs"])
    assert res.labels.dtype == torch.int32 and np.array_equal(res.labels.cpu().numpy(), out["labels"])
    assert np.array_equal(trk.keys.cpu().numpy(), orc.keys)
    assert res.out_of_grid == out["out_of_grid"]
    assert res.status == out["status"] and res.ids == out["ids"] and res.new == out["new"] and res.merged == out["merged"]
    assert trk.class_of == orc.class_of and trk.next_id == orc.next_id and sorted(trk.boxes) == sorted(orc.class_of)
    return res, out


def run_sequence(frames, wide=False, **kw):
    shift = 1 if wide else 0
    trk, orc = make_tracker(shift, **kw), make_oracle(shift, **kw)
    return trk, [put_both(trk, orc, f, wide) for f in frames]


@pytest.mark.parametrize("wide", [False, True], ids=["u16", "f32-i32"])
def test_main_sequence_equals_the_oracle(wide):
    """Empty state with every non-match status; scrambled rows from a moved pose; class mismatch, below threshold and shared match -
    in both input types (the wide one with det_shift = 1, a raw row of -1 and a NaN depth)."""
    frames = tc.main_sequence()
    trk, ((one, _), (two, _), (three, _)) = run_sequence(frames, wide)
    row = {name: d for d, name in enumerate(tc.ORDER_1, 1)}
    assert one.status == {0: to.BACKGROUND, row["A"]: to.NEW, row["B"]: to.NEW, row["C"]: to.NEW, row["BG"]: to.BACKGROUND, row["THIN"]: to.SMALL,
                          row["FEW"]: to.FEW_POINTS, row["TINY"]: to.NEW_NO_BOX, row["D"]: to.NEW, row["E"]: to.NEW}
    assert one.new == [1, 2, 3, 5, 6] and 4 not in trk.boxes
    row = {name: d for d, name in enumerate(tc.ORDER_2, 1)}
    assert two.ids == {row[n]: i for n, i in tc.IDS.items()} and not two.new and two.merged == [1, 2, 3, 5, 6]
    lab = two.labels.cpu().numpy()
    for name, i in tc.IDS.items():
        assert set(lab[frames[1][0] == row[name]].tolist()) == {i, -1}, name
    assert three.status == {0: to.BACKGROUND, 1: to.NEW, 2: to.NEW, 3: to.MERGED, 4: to.MERGED, 5: to.MERGED}
    assert three.ids == {1: 7, 2: 8, 3: 1, 4: 1, 5: 2} and three.merged == [1, 2]
    # the shared match: both halves of A put their inside points into id 1's cloud (put_both holds the key state to the checker's)
    assert three.rows[3][3] == three.rows[4][3] == 1 and three.rows[3][6] > 0 and three.rows[4][6] > 0
    known = trk.box_table[:, 15].cpu().numpy() != 0
    assert np.flatnonzero(known).tolist() == sorted(trk.boxes) == [1, 2, 3, 5, 6, 7, 8]


def test_radius_six_halo_equals_the_oracle():
    """The first frame at the reference's erosion radius: the halo is as wide as it gets but for two pixels, and every mask erodes to
    a few pixels or to nothing."""
    trk, ((one, out),) = run_sequence(tc.main_sequence()[:1], erode_radius=6)
    assert set(one.status.values()) == {to.BACKGROUND, to.SMALL} and one.rows[1:, 7].max() == 2 * 5 and not trk.boxes and trk.next_id == 1


def test_overlapping_candidates_the_lower_id_wins():
    trk, (_, (two, _), (three, _)) = run_sequence(tc.overlap_sequence())
    assert two.ids == {1: 2}
    (_, i1, n1), (_, i2, n2) = three.pairs.tolist()
    assert (i1, i2) == (1, 2) and n2 > n1 and three.status[1] == to.MERGED and three.ids == {1: 1} and three.rows[1][6] == n1


def test_more_pairs_than_the_lds_table_holds():
    """The pairs that find no slot in the LDS table of the first tile's workgroup go to the global table directly."""
    from vmap_amd import _lib
    trk, (_, _, (three, _)) = run_sequence(tc.overflow_sequence(_lib.TRACK_PAIR_SLOTS))
    tile = three.pairs[three.pairs[:, 0] <= 12]
    assert len(tile) == 120 > _lib.TRACK_PAIR_SLOTS and (tile[_lib.TRACK_PAIR_SLOTS + 4:, 2] > 0).sum() >= 4
    assert sorted(trk.boxes) == list(range(1, 11))


def test_key_grid_edge():
    frame = tc.edge_frame()
    edge = 32768 * tc.SETTINGS["voxel_size"]
    res, _ = put_both(make_tracker(), make_oracle(), frame[:3] + (tc.pose(tx=edge - 0.3),))
    assert res.out_of_grid > 0 and res.new
    far = make_tracker()
    res, _ = put_both(far, make_oracle(), frame[:3] + (tc.pose(tx=edge + 50.0),))
    assert res.out_of_grid > 0 and len(far.keys) == 0 and not far.boxes and far.next_id == 6      # every NEW row lost its id


def test_registered_boxes_are_the_search_on_the_decoded_cloud_plus_the_margin():
    from vmap_amd import bounds, instances
    trk, _ = run_sequence(tc.main_sequence())
    table = trk.box_table.cpu().numpy()
    for i, box in trk.boxes.items():
        pts = trk.points(i)
        keys = trk.keys[(trk.keys >> 48) == i].cpu().numpy()
        assert np.array_equal(pts.cpu().numpy(), to.fo.key_points(keys, trk.voxel_size)) and len(keys) >= 4
        again = bounds.oriented_bounds(pts, backend="hip", min_extent=trk.min_extent)[0]
        assert np.array_equal(again.center, box.center) and np.array_equal(again.R, box.R) and np.array_equal(again.extent, box.extent)
        assert again.extent.min() >= trk.min_extent
        assert np.array_equal(table[i], instances.box_row(again, 0.875 * trk.voxel_size))
    assert np.flatnonzero(table[:, 15]).tolist() == sorted(trk.boxes)


def test_two_fresh_trackers_agree_byte_for_byte():
    a, ra = run_sequence(tc.main_sequence(), wide=True)
    b, rb = run_sequence(tc.main_sequence(), wide=True)
    for (x, _), (y, _) in zip(ra, rb):
        assert torch.equal(x.labels, y.labels) and x.rows.tobytes() == y.rows.tobytes() and x.pairs.tobytes() == y.pairs.tobytes()
    assert torch.equal(a.keys, b.keys) and a.box_table.cpu().numpy().tobytes() == b.box_table.cpu().numpy().tobytes()


def test_labels_hand_off_to_frame_ingest():
    """res.labels into FrameIngest.put gives the boxes the ingest checker computes from the oracle's labels."""
    from vmap_amd import ingest, keyframes
    frames = tc.main_sequence()
    trk, results = run_sequence(frames)
    store = keyframes.FrameStore(2, tc.W, tc.H, device=DEV)
    s = tc.SETTINGS
    ing = ingest.FrameIngest(store, s["depth_scale"], s["max_depth"], background_classes=(), min_box=-1, max_ids=s["max_ids"] + 1)
    rgb = np.random.default_rng(1).integers(0, 256, (tc.H, tc.W, 3), dtype=np.uint8)
    res, out = results[1]
    depth, t_wc = frames[1][2], frames[1][3]
    got = ing.put(torch.from_numpy(rgb), torch.from_numpy(depth), res.labels, None, t_wc, 5)
    want = io.ingest(rgb, depth, out["labels"], None, s["depth_scale"], s["max_depth"], (), 0.2, -1, s["max_ids"] + 1)
    assert np.array_equal(got.rows, want["rows"]) and -1 in got.ids and 1 in got.ids
    bd = io.bbox_dict(want["rows"])
    assert got.ids == list(bd) and all(got.bbox[i].tolist() == [float(x) for x in bd[i]] for i in bd)
    assert np.array_equal(store.inst[got.slot].cpu().numpy(), want["inst"])


def test_errors_leave_the_state_untouched():
    """A row outside [0, max_det - 1], a row without a class, more pairs than max_pairs and an id that would reach max_ids raise
    ValueError and change neither the keys, the box table, class_of nor next_id; the tracker goes on as if nothing had happened."""
    frames = tc.main_sequence()
    kw = dict(max_ids=8, max_pairs=12)                        # frame 1 takes ids 1 .. 6; frame 2 needs 9 pairs; frame 3 two more ids
    trk, orc = make_tracker(**kw), make_oracle(**kw)
    put_both(trk, orc, frames[0])
    keys, table, class_of = trk.keys.clone(), trk.box_table.clone(), dict(trk.class_of)
    rows, classes, depth, t_wc = frames[1]
    d, det, _ = tc.typed(rows, depth, False)
    bad = det.copy()
    bad[0, 0] = tc.SETTINGS["max_det"]
    with pytest.raises(ValueError, match="outside"):
        trk.put(d, bad, classes, t_wc)
    with pytest.raises(ValueError, match="no entry in det_classes"):
        trk.put(d, det, classes[:5], t_wc)
    with pytest.raises(ValueError, match="pairs"):
        trk.put(d, det, [0] + [50] * 8, t_wc)                 # 8 rows x 2 instances of class 50
    d3, det3, _ = tc.typed(frames[2][0], frames[2][2], False)
    with pytest.raises(ValueError, match="max_ids"):
        trk.put(d3, det3, frames[2][1], frames[2][3])
    assert torch.equal(trk.keys, keys) and torch.equal(trk.box_table, table) and trk.class_of == class_of and trk.next_id == 7 and len(trk.boxes) == 5
    put_both(trk, orc, frames[1])                             # and the tracker goes on as if nothing had happened
