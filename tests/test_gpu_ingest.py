"""GPU tier of frame ingest (vmap_amd/ingest.py; csrc/ingest_kernels.h): exact equality - the table of ids and all three images of the
slot - with the fixtures the reference's own loader produced (tests/golden/ingest_*.npz) and with the numpy checker
(tests/ingest_oracle.py) for what the reference cannot produce.  Everything is integer or one float32 product: there is no tolerance
anywhere.  Frames are at most 200 x 150; the sizes are the ones where the kernels take another path: the 64 x 64 tile of ingest_write
and the 2048-pixel share of an ingest_stats workgroup on both sides, a one-pixel frame, more ids than the LDS table has slots."""
import numpy as np
import pytest
import torch

import ingest_oracle as io
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FIXTURES = ("ingest_rects", "ingest_noise", "ingest_imap")
TYPES = [(np.uint16, np.uint16), (np.uint16, np.int32), (np.float32, np.uint16), (np.float32, np.int32)]     # depth, labels


def make_frame(W, H, seed, n_ids=12, cell=(5, 9)):
    """A random frame [H, W]: ids on a coarse grid (several per tile), one class per id, 16-bit depth."""
    rng = np.random.default_rng(seed)
    labels = np.concatenate([[0], rng.choice(np.arange(1, 900), n_ids - 1, replace=False)])
    classes = rng.choice(np.array([3, 7, 11, 20, 40, 93]), labels.size)
    cells = rng.integers(0, labels.size, (-(-H // cell[0]), -(-W // cell[1])))
    idx = np.repeat(np.repeat(cells, cell[0], axis=0), cell[1], axis=1)[:H, :W]
    return dict(rgb=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), depth=rng.integers(0, 65536, (H, W)).astype(np.uint16),
                inst=labels[idx].astype(np.uint16), sem=classes[idx].astype(np.uint16))


SETTINGS = dict(depth_scale=1.0 / 6553.5, max_depth=8.0, background=(40, 93), bbox_scale=0.2, min_box=10, max_ids=1024)


def settings_of(g):
    return dict(depth_scale=float(g["depth_scale"]), max_depth=float(g["max_depth"]), background=tuple(g["background"].tolist()),
                bbox_scale=float(g["bbox_scale"]), min_box=int(g["min_box"]), max_ids=1024)


def make_ingest(W, H, s, capacity=2):
    from vmap_amd import ingest, keyframes
    store = keyframes.FrameStore(capacity, W, H, device=DEV)
    return ingest.FrameIngest(store, s["depth_scale"], s["max_depth"], background_classes=s["background"], bbox_scale=s["bbox_scale"],
                              min_box=s["min_box"], max_ids=s["max_ids"])


def typed(frame, depth_t=np.uint16, label_t=np.uint16):
    cast = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(t))
    return cast(frame["rgb"], np.uint8), cast(frame["depth"], depth_t), cast(frame.get("inst"), label_t), cast(frame.get("sem"), label_t)


def device_table(ing, slot, frame, depth_t=np.uint16, label_t=np.uint16):
    """The launches alone (FrameIngest.enqueue), without put's error handling -> (rows int32 [n, 8], overflow)."""
    rgb, depth, inst, sem = (None if t is None else t.to(DEV) for t in typed(frame, depth_t, label_t))
    ing.enqueue(slot, rgb, depth, inst, sem)
    head = ing._rows_dev.cpu().numpy()
    return head[2:2 + 8 * int(head[0])].reshape(-1, 8).copy(), int(head[1])


def assert_slot_equals(store, slot, o):
    assert np.array_equal(store.rgbx[slot].cpu().numpy(), o["rgbx"])
    assert np.array_equal(store.depth[slot].cpu().numpy().view(np.uint32), o["depth"].view(np.uint32))
    assert np.array_equal(store.inst[slot].cpu().numpy(), o["inst"])


def check_against_oracle(frame, s, depth_t=np.uint16, label_t=np.uint16, t_wc=None):
    H, W = frame["rgb"].shape[:2]
    ing = make_ingest(W, H, s)
    o = io.ingest(frame["rgb"], frame["depth"], frame.get("inst"), frame.get("sem"), s["depth_scale"], s["max_depth"], s["background"],
                  s["bbox_scale"], s["min_box"], s["max_ids"])
    t_wc = np.eye(4, dtype=np.float32) if t_wc is None else t_wc
    res = ing.put(*typed(frame, depth_t, label_t), torch.from_numpy(t_wc), 7)
    assert np.array_equal(res.rows, o["rows"]), (res.rows, o["rows"])
    assert_slot_equals(ing.store, res.slot, o)
    assert np.array_equal(ing.store.t_wc[res.slot].cpu().numpy(), t_wc) and ing.store.frame_of_slot[res.slot] == 7
    bd = io.bbox_dict(o["rows"])
    assert res.ids == list(bd) and all(res.bbox[i].dtype == torch.float32 and res.bbox[i].tolist() == [float(x) for x in bd[i]] for i in bd)
    assert res.counts == {int(r[0]): int(r[2]) for r in o["rows"]} and res.status == {int(r[0]): int(r[1]) for r in o["rows"]}
    return ing, res, o


@pytest.mark.parametrize("types", TYPES, ids=["d16-l16", "d16-l32", "d32-l16", "d32-l32"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_reproduced_exactly(name, types):
    """The table and the three images against the checker AND against what dataset.Replica.__getitem__ returned, in all four
    combinations of input types."""
    g = load_golden(name)
    imap = bool(g["imap"])
    frame = dict(rgb=g["rgb"], depth=g["depth"], inst=None if imap else g["inst"], sem=None if imap else g["sem"])
    ing, res, _ = check_against_oracle(frame, settings_of(g), *types)
    st = ing.store
    assert np.array_equal(st.inst[res.slot].cpu().numpy(), g["ref_obj"])
    assert np.array_equal(st.rgbx[res.slot, :, :, :3].cpu().numpy(), g["ref_image"])
    assert np.array_equal(st.depth[res.slot].cpu().numpy().view(np.uint32), g["ref_depth"].view(np.uint32))
    assert res.ids == g["ref_bbox_ids"].tolist()
    assert np.array_equal(np.stack([res.bbox[i].numpy() for i in res.ids]), g["ref_bbox"].astype(np.float32))


# the 64 x 64 tile of ingest_write on both sides in each dimension, one tile plus one pixel, one pixel; 2048 pixels per ingest_stats
# workgroup: 64 x 32 is exactly one, 65 x 32 one more pixel; rows that straddle a wave (widths that are no multiple of 64)
SIZES = [(1, 1), (63, 63), (64, 64), (65, 65), (64, 65), (65, 64), (64, 32), (65, 32), (200, 150), (3, 131)]


@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_frame_sizes_around_the_tiles(W, H):
    check_against_oracle(make_frame(W, H, seed=W * 1000 + H, cell=(7, 13)), dict(SETTINGS, min_box=3), np.uint16, np.int32)


def test_more_ids_in_a_workgroup_than_the_lds_table_holds():
    """A one-pixel checkerboard of 200 ids over 128 x 32: each of the two ingest_stats workgroups meets every id, 64 find a slot of its
    LDS table, the others go to the global table directly - and the result is the checker's."""
    W, H = 128, 32
    v, u = np.mgrid[0:H, 0:W]
    frame = make_frame(W, H, seed=5)
    frame["inst"] = (1 + (u + 7 * v) % 200).astype(np.uint16)
    frame["sem"] = (frame["inst"] % 50).astype(np.uint16)
    _, res, _ = check_against_oracle(frame, dict(SETTINGS, background=(3, 4, 5)))
    assert len(res.rows) == 201 and set(res.counts.values()) >= {20, 21}


def rects():
    g = load_golden("ingest_rects")
    return dict(rgb=g["rgb"], depth=g["depth"], inst=g["inst"], sem=g["sem"]), settings_of(g)


def test_largest_id_and_one_past_it():
    """Id 300 is the last row at max_ids = 302; at 301 it has no row: its pixels are the overflow, put raises and the slot stays free."""
    frame, s = rects()
    check_against_oracle(frame, dict(s, max_ids=302))
    ing = make_ingest(64, 48, dict(s, max_ids=301))
    pixels = int((frame["inst"] == 300).sum())
    rows, overflow = device_table(ing, 0, frame)
    o = io.ingest(frame["rgb"], frame["depth"], frame["inst"], frame["sem"], s["depth_scale"], s["max_depth"], s["background"], s["bbox_scale"],
                  s["min_box"], 301)
    assert overflow == pixels == o["overflow"] and np.array_equal(rows, o["rows"]) and 300 not in rows[:, 0]
    assert_slot_equals(ing.store, 0, o)
    with pytest.raises(ValueError, match=f"{pixels} pixels.*max_ids"):
        ing.put(*typed(frame), torch.eye(4), 3)
    assert ing.store.frame_of_slot == [None, None] and ing.store.free_slot() == 0


def test_every_uint16_label_has_a_row_at_the_largest_table():
    """max_ids = 65537: id 65535 is an ordinary row (and the table is kept in one copy instead of several)."""
    frame, s = rects()
    check_against_oracle(frame, dict(s, max_ids=4097), np.float32, np.int32)                # the first size with one copy
    frame = dict(frame, inst=np.where(frame["inst"] == 300, 65535, frame["inst"]).astype(np.uint16))
    _, res, _ = check_against_oracle(frame, dict(s, max_ids=65537))
    assert res.ids[-1] == 65535 and res.status[65535] == io.KEPT


def test_unsure_label_is_an_ordinary_row():
    frame, s = rects()
    inst = frame["inst"].astype(np.int32)
    inst[10:30, 45:64] = -1
    sem = frame["sem"].astype(np.int32)
    sem[inst == -1] = -1
    _, res, _ = check_against_oracle(dict(frame, inst=inst, sem=sem), s, np.uint16, np.int32)
    assert res.rows[0, 0] == -1 and res.status[-1] == io.KEPT and -1 in res.bbox
    _, res, _ = check_against_oracle(dict(frame, inst=inst, sem=sem), dict(s, background=s["background"] + (-1,)), np.float32, np.int32)
    assert res.status[-1] == io.BACKGROUND


def test_two_classes_on_one_instance_raise():
    """MIXED: a second class inside a run of one row (the lanes of a run that disagree with its leader) and on a row of its own."""
    frame, s = rects()
    sem = frame["sem"].copy()
    sem[7, 9:12] = 21                      # inside id 1's rows
    sem[40:42, 3:20] = 41                  # whole rows of id 2
    frame = dict(frame, sem=sem)
    ing = make_ingest(64, 48, s)
    rows, overflow = device_table(ing, 0, frame)
    o = io.ingest(frame["rgb"], frame["depth"], frame["inst"], sem, s["depth_scale"], s["max_depth"], s["background"], s["bbox_scale"], s["min_box"])
    assert overflow == 0 and np.array_equal(rows, o["rows"])
    assert {int(r[0]) for r in rows if r[1] == io.MIXED} == {1, 2}
    assert_slot_equals(ing.store, 0, o)
    with pytest.raises(ValueError, match="instance id 1 "):
        ing.put(*typed(frame), torch.eye(4), 3)
    assert ing.store.free_slot() == 0


def test_zero_margin_is_background():
    frame, s = rects()
    _, res, _ = check_against_oracle(frame, dict(s, bbox_scale=0.05))
    assert res.status[4] == io.ZERO_MARGIN and res.status[3] == io.SMALL and 4 not in res.ids          # 0.025 * 11 truncates to 0


def test_every_instance_background():
    frame, s = rects()
    _, res, o = check_against_oracle(frame, dict(s, background=tuple(sorted(set(frame["sem"].reshape(-1).tolist())))))
    assert res.ids == [0] and not o["inst"].any() and res.bbox[0].tolist() == [0.0, 64.0, 0.0, 48.0]


def test_filtered_label_image_mode():
    """background_classes=(), min_box=-1, sem=None: the second half of the reference's ScanNet loader, against the checker only."""
    frame = make_frame(150, 70, seed=11, n_ids=20, cell=(4, 6))
    frame["sem"] = None
    frame["inst"][:2, :3] = 950            # a 3 x 2 instance: margin 0 -> background
    _, res, _ = check_against_oracle(frame, dict(SETTINGS, background=(), min_box=-1), np.float32, np.uint16)
    assert res.status[950] == io.ZERO_MARGIN and io.SMALL not in res.status.values()


def test_two_runs_are_bit_identical_and_the_slot_behaves_as_puts():
    frame = make_frame(200, 150, seed=3, n_ids=60, cell=(5, 7))
    ing = make_ingest(200, 150, SETTINGS, capacity=3)
    st = ing.store
    a = ing.put(*typed(frame), torch.eye(4), 0)
    b = ing.put(*typed(frame), torch.eye(4), 1)
    assert (a.slot, b.slot) == (0, 1) and st.refs == [0, 0, 0] and st.frame_of_slot == [0, 1, None]
    assert np.array_equal(a.rows, b.rows)
    for t in (st.rgbx, st.depth, st.inst):
        assert torch.equal(t[0], t[1])
    st.retain(b.slot)
    st.collect()                            # frame 0 was kept by nobody
    assert st.frame_of_slot == [None, 1, None]
    c = ing.put(*typed(frame), torch.eye(4), 2)
    assert c.slot == 0 and np.array_equal(c.rows, a.rows)
    st.release(b.slot)
    assert st.frame_of_slot == [2, None, None]
    ing.put(*typed(frame), torch.eye(4), 3)
    ing.put(*typed(frame), torch.eye(4), 4)
    with pytest.raises(RuntimeError, match="full"):
        ing.put(*typed(frame), torch.eye(4), 5)


def test_ingested_frame_feeds_the_sampler_as_a_put_frame_does():
    """End to end: FrameIngest.put -> ObjectKeyframes -> FrameSampler equals, bit for bit, the same sampler over a store filled by
    FrameStore.put with the checker's images and boxes, at the same seed."""
    from vmap_amd import keyframes, sampler
    g = load_golden("ingest_rects")
    frame, s = rects()
    t_wc = np.eye(4, dtype=np.float32)
    t_wc[:3, 3] = [0.1, -0.2, 0.3]
    ing, res, o = check_against_oracle(frame, s, t_wc=t_wc)
    W, H = 64, 48
    plain = keyframes.FrameStore(2, W, H, device=DEV)
    slot = plain.put(torch.from_numpy(o["rgbx"][..., :3].copy()), torch.from_numpy(o["depth"]), torch.from_numpy(o["inst"]), torch.from_numpy(t_wc), 7)
    bd = io.bbox_dict(o["rows"])
    outs = []
    for store, sl, boxes in ((ing.store, res.slot, res.bbox), (plain, slot, {i: [float(x) for x in b] for i, b in bd.items()})):
        oks = [keyframes.ObjectKeyframes(store, i, sl, boxes[i], keyframe_buffer_size=3) for i in res.ids]
        smp = sampler.FrameSampler(W, H, 4, 6, 2, 5, 60.0, 55.0, 31.5, 23.5, min_depth=0.0, surface_eps=0.1, stop_eps=0.05, device=DEV, seed=9)
        smp.set_objects([ok.sampler_entry() for ok in oks])
        outs.append({k: v.cpu().numpy() for k, v in smp.sample().items()})
        assert store.refs[sl] == len(res.ids)
    assert res.ids == g["ref_bbox_ids"].tolist() and len(res.ids) == 6
    for k in outs[0]:
        assert np.array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8)), k
    assert outs[0]["depth_mask"].any() and outs[0]["sem"].max() >= 1
