"""GPU tier of the instance filter (vmap_amd/instances.py; csrc/filter_kernels.h): exact equality - the table of ids, the sorted key
set and the label image - with the numpy checker (tests/filter_oracle.py), which is handed the device's own float32 box table at
every frame, so that the box search (covered by the bounds tests) is out of the comparison.  Everything is integer or float32 with
every rounding pinned: there is no tolerance anywhere.  The frames are tests/filter_cases.py's: 75 x 53, a multiple of no tile
dimension (two filter_stats tiles across, four down; four blocks of the linear kernels, the last one partial)."""
import numpy as np
import pytest
import torch

import filter_cases as fc
import filter_oracle as fo
import ingest_oracle as io

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_filter(radius=6, id_shift=0, **kw):
    from vmap_amd import instances
    s = dict(fc.SETTINGS, **kw)
    return instances.InstanceFilter(fc.W, fc.H, fc.INTRINSICS, s["depth_scale"], s["max_depth"], background_classes=s["background"],
                                    min_pixels=s["min_pixels"], min_points=s["min_points"], erode_radius=radius, voxel_size=s["voxel_size"],
                                    id_shift=id_shift, max_ids=s["max_ids"], device=DEV)


def make_oracle(radius=6, id_shift=0, **kw):
    s = dict(fc.SETTINGS, **kw)
    return fo.Filter(fc.W, fc.H, fc.INTRINSICS, s["depth_scale"], s["max_depth"], s["background"], s["min_pixels"], s["min_points"], radius,
                     s["voxel_size"], id_shift, s["max_ids"])


def put_both(flt, orc, frame, wide=False):
    """One frame through the device and through the checker (with the box table the device judged it by); asserts equality of the
    rows, the labels, the key state and the counters.  -> (FilterResult, oracle dict)"""
    ids, sem, depth, t_wc = frame
    d, i, s, _ = fc.typed(ids, sem, depth, wide)
    table = flt.box_table.cpu().numpy().copy()
    res = flt.put(torch.from_numpy(d), torch.from_numpy(i), torch.from_numpy(s), t_wc)
    out = orc.put(d, i, s, t_wc, table)
    assert np.array_equal(res.rows, out["rows"]), (res.rows, out["rows"])
    assert res.labels.dtype == torch.int32 and np.array_equal(res.labels.cpu().numpy(), out["labels"])
    assert np.array_equal(flt.keys.cpu().numpy(), orc.keys)
    assert res.out_of_grid == out["out_of_grid"]
    assert res.status == {int(r[0]): int(r[1]) for r in out["rows"]} and res.counts == {int(r[0]): int(r[3]) for r in out["rows"]}
    assert res.classes == {int(r[0]): int(r[2]) for r in out["rows"]}
    assert res.new == [int(r[0]) for r in out["rows"] if r[1] == fo.NEW] and res.merged == [int(r[0]) for r in out["rows"] if r[1] == fo.MERGED]
    return res, out


@pytest.mark.parametrize("wide", [False, True], ids=["u16", "f32-i32"])
@pytest.mark.parametrize("radius", [6, 2])
def test_one_frame_equals_the_oracle(radius, wide):
    """(a) Every case of tests/filter_cases.base_frame on an empty state, at both radii and in both input types (the wide one with
    id_shift = 1, a raw id of -1 and a NaN depth)."""
    ids, sem, depth = fc.base_frame()
    shift = 1 if wide else 0
    flt, orc = make_filter(radius, shift), make_oracle(radius, shift)
    res, out = put_both(flt, orc, (ids, sem, depth, fc.pose()), wide)
    want = {0: fo.BACKGROUND, fc.ID_NEW: fo.NEW, fc.ID_CORNER: fo.NEW, fc.ID_FILL: fo.BACKGROUND, fc.ID_LEFT: fo.NEW, fc.ID_RIGHT: fo.NEW,
            fc.ID_FEW: fo.FEW_POINTS}
    want.update({fc.ID_STRIP: fo.SMALL, fc.ID_RIM: fo.NEW_NO_BOX, fc.ID_LAST: fo.SMALL} if radius == 6 else
                {fc.ID_STRIP: fo.NEW, fc.ID_RIM: fo.NEW, fc.ID_LAST: fo.NEW})
    assert res.status == want
    assert sorted(flt.boxes) == res.new and len(flt.keys) > 0
    known = flt.box_table[:, 15].cpu().numpy() != 0
    assert np.flatnonzero(known).tolist() == res.new


def run_sequence(wide=False, frames=None):
    shift = 1 if wide else 0
    flt, orc = make_filter(6, shift), make_oracle(6, shift)
    results = [put_both(flt, orc, f, wide) for f in (frames or fc.sequence())]
    return flt, results


def test_three_frames_with_a_moving_pose():
    """(b) Every status occurs; the MERGED frame has both id and -1 pixels; an id entirely outside its box is -1 everywhere."""
    frames = fc.sequence()
    flt, results = run_sequence(frames=frames)
    seen = set()
    for res, _ in results:
        seen |= set(res.status.values())
    assert seen == {fo.NEW, fo.MERGED, fo.UNSURE, fo.SMALL, fo.FEW_POINTS, fo.BACKGROUND, fo.NEW_NO_BOX}
    res2 = results[1][0]
    assert res2.status[fc.ID_NEW] == fo.MERGED and res2.status[fc.ID_CORNER] == fo.UNSURE and res2.new == [fc.ID_LATE]
    lab = res2.labels.cpu().numpy()
    own = lab[frames[1][0] == fc.ID_NEW]
    assert (own == fc.ID_NEW).any() and (own == -1).any() and set(own.tolist()) == {fc.ID_NEW, -1}
    assert (lab[frames[1][0] == fc.ID_CORNER] == -1).all()
    assert results[2][0].status[fc.ID_LATE] == fo.MERGED and fc.ID_CORNER not in results[2][0].merged
    assert sorted(flt.boxes) == [fc.ID_NEW, fc.ID_CORNER, fc.ID_LEFT, fc.ID_RIGHT, fc.ID_LATE]


def test_margin_keeps_every_merged_point_inside_the_next_box():
    """(c) The same frame twice: every id that was NEW is MERGED, and no valid pixel of the first pass's eroded region is -1."""
    ids, sem, depth = fc.base_frame()
    frame = (ids, sem, depth, fc.pose(0.3, -0.2, 0.1, 0.4))
    flt, orc = make_filter(), make_oracle()
    first, _ = put_both(flt, orc, frame)
    second, _ = put_both(flt, orc, frame)
    assert first.new and second.merged == first.new and not second.new
    lab = second.labels.cpu().numpy()
    valid = fo.depth_of(depth, fc.SETTINGS["depth_scale"], fc.SETTINGS["max_depth"]) > 0
    for i in first.new:
        core = fo.erode(ids == i, 6) & valid
        assert core.any() and (lab[core] == i).all(), i
    assert (lab == -1).any()                                  # the masks' rims were never merged: outside


def test_registered_boxes_are_the_search_on_the_decoded_cloud_plus_the_margin():
    """(d)"""
    from vmap_amd import bounds, instances
    flt, _ = run_sequence()
    table = flt.box_table.cpu().numpy()
    for i, box in flt.boxes.items():
        pts = flt.points(i)
        keys = flt.keys[(flt.keys >> 48) == i].cpu().numpy()
        assert np.array_equal(pts.cpu().numpy(), fo.key_points(keys, flt.voxel_size)) and len(keys) >= 4
        again = bounds.oriented_bounds(pts, backend="hip", min_extent=0.0)[0]
        assert np.array_equal(again.center, box.center) and np.array_equal(again.R, box.R) and np.array_equal(again.extent, box.extent)
        assert np.array_equal(table[i], instances.box_row(again, 0.875 * flt.voxel_size))
        assert np.array_equal(table[i, 12:15], (0.5 * again.extent + 0.875 * flt.voxel_size).astype(np.float32))
    assert np.flatnonzero(table[:, 15]).tolist() == sorted(flt.boxes)


def test_two_fresh_filters_agree_byte_for_byte():
    """(e)"""
    a, ra = run_sequence(wide=True)
    b, rb = run_sequence(wide=True)
    for (x, _), (y, _) in zip(ra, rb):
        assert torch.equal(x.labels, y.labels) and x.rows.tobytes() == y.rows.tobytes()
    assert torch.equal(a.keys, b.keys) and a.box_table.cpu().numpy().tobytes() == b.box_table.cpu().numpy().tobytes()


def test_labels_hand_off_to_frame_ingest():
    """(f) res.labels into FrameIngest.put gives the boxes the ingest checker computes from the oracle's labels."""
    from vmap_amd import ingest, keyframes
    frames = fc.sequence()
    flt, results = run_sequence(frames=frames)
    store = keyframes.FrameStore(2, fc.W, fc.H, device=DEV)
    ing = ingest.FrameIngest(store, fc.SETTINGS["depth_scale"], fc.SETTINGS["max_depth"], background_classes=(), min_box=-1, max_ids=fc.MAX_IDS + 1)
    rgb = np.random.default_rng(1).integers(0, 256, (fc.H, fc.W, 3), dtype=np.uint8)
    res, out = results[1]
    depth, t_wc = frames[1][2], frames[1][3]
    got = ing.put(torch.from_numpy(rgb), torch.from_numpy(depth), res.labels, None, t_wc, 5)
    want = io.ingest(rgb, depth, out["labels"], None, fc.SETTINGS["depth_scale"], fc.SETTINGS["max_depth"], (), 0.2, -1, fc.MAX_IDS + 1)
    assert np.array_equal(got.rows, want["rows"]) and -1 in got.ids and fc.ID_NEW in got.ids
    bd = io.bbox_dict(want["rows"])
    assert got.ids == list(bd) and all(got.bbox[i].tolist() == [float(x) for x in bd[i]] for i in bd)
    assert np.array_equal(store.inst[got.slot].cpu().numpy(), want["inst"])


def test_errors_leave_the_state_untouched():
    """(g) A mixed class and an id out of range raise ValueError and change neither the keys nor the box table; a point beyond the key
    range is counted and is no error."""
    frames = fc.sequence()
    flt, orc = make_filter(), make_oracle()
    put_both(flt, orc, frames[0])
    keys, table = flt.keys.clone(), flt.box_table.clone()
    ids, sem, depth, t_wc = frames[1]
    sem_bad = sem.copy()
    sem_bad[3, 3] += 1
    d, i, s, _ = fc.typed(ids, sem_bad, depth, False)
    with pytest.raises(ValueError, match="more than one semantic class"):
        flt.put(d, i, s, t_wc)
    ids_bad = ids.copy()
    ids_bad[0, 0] = fc.MAX_IDS
    d, i, s, _ = fc.typed(ids_bad, sem, depth, False)
    with pytest.raises(ValueError, match="outside"):
        flt.put(d, i, s, t_wc)
    assert torch.equal(flt.keys, keys) and torch.equal(flt.box_table, table) and len(flt.boxes) == 4
    put_both(flt, orc, frames[1])                             # and the filter goes on as if nothing had happened
    far = make_filter()
    res, out = put_both(far, make_oracle(), (frames[0][0], frames[0][1], frames[0][2], fc.pose(tx=700.0)))
    assert res.out_of_grid > 0 and len(far.keys) == 0 and not far.boxes
    near = make_filter()
    res, _ = put_both(near, make_oracle(), (frames[0][0], frames[0][1], frames[0][2], fc.pose(tx=655.2)))     # the grid's end (655.36 m) crosses the eroded regions
    assert res.out_of_grid > 0 and len(near.keys) > 0
