"""Generate the ingest fixtures by running the REAL reference loader (dataset.Replica.__getitem__, unmodified) on synthetic frames.

Authoring container only (needs /root/reference).  ``dataset.py`` imports cv2 / imgviz / open3d / torchvision at module level
(none installed): ``cv2.imread`` serves the synthetic arrays from a dict, ``cv2.cvtColor`` reverses the channel axis,
``torchvision.transforms.Compose`` applies a list of callables, the rest are mocks - the device tests/golden/make_sampler_goldens.py
uses for the sampler.  Nothing of the reference is copied: the stored arrays are the inputs made here and what its loader returned
for them (``image``, ``depth``, ``obj``, ``bbox_dict``).  tests/ingest_oracle.py must already agree (asserted below).
"""
from __future__ import annotations

import os
import sys
import tempfile
import types
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import ingest_oracle as io  # noqa: E402

REF = "/root/reference"
FILES = {}                                  # basename prefix -> array, what the stubbed cv2.imread serves

DEPTH_SCALE, MAX_DEPTH = 1.0 / 6553.5, 8.0  # the reference's Replica settings


def import_reference_dataset():
    cv2 = mock.MagicMock()

    def imread(path, flag=None):
        name = os.path.basename(path)
        for prefix, arr in FILES.items():
            if name.startswith(prefix + "_"):
                return arr.copy()
        raise FileNotFoundError(path)

    cv2.imread = imread
    cv2.cvtColor = lambda img, code: img[..., ::-1]
    sys.modules["cv2"] = cv2
    for name in ("imgviz", "open3d"):
        sys.modules.setdefault(name, mock.MagicMock())
    try:
        import functorch  # noqa: F401
    except Exception:      # noqa: BLE001
        sys.modules["functorch"] = mock.MagicMock()

    class Compose:
        def __init__(self, fns):
            self.fns = list(fns)

        def __call__(self, x):
            for f in self.fns:
                x = f(x)
            return x

    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.Compose = Compose
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.transforms"] = tv.transforms
    sys.path.insert(0, REF)
    import dataset as ref_dataset
    assert os.path.dirname(ref_dataset.__file__) == REF
    return ref_dataset


def paint(inst, sem, idv, cls, rows, cols):
    inst[rows[0]:rows[1], cols[0]:cols[1]] = idv
    sem[rows[0]:rows[1], cols[0]:cols[1]] = cls


def colour_and_depth(rng, W, H):
    """Random, but compressible (the fixtures stay small): colours constant over 3 x 3 blocks, 1024 depth levels up to 10 m, a
    fifth of them past max_depth."""
    rgb = np.repeat(np.repeat(rng.integers(0, 256, (-(-H // 3), -(-W // 3), 3), dtype=np.uint8), 3, axis=0), 3, axis=1)[:H, :W]
    depth = (rng.integers(0, 1024, (H, W)) * 64).astype(np.uint16)
    return np.ascontiguousarray(rgb), depth


def rects_frame():
    """64 x 48: a kept rectangle, one of a background class, extents of exactly 10 (dropped) and 11 (kept), one touching two borders,
    one id above 255, one instance partly overwritten by another."""
    W, H = 64, 48
    rng = np.random.default_rng(101)
    inst, sem = np.zeros((H, W), np.uint16), np.full((H, W), 93, np.uint16)      # the wall: a background class
    paint(inst, sem, 1, 20, (5, 25), (5, 25))            # 20 x 20: kept
    paint(inst, sem, 2, 40, (30, 46), (2, 21))           # floor: background
    paint(inst, sem, 3, 7, (2, 17), (30, 40))            # u extent exactly 10: dropped
    paint(inst, sem, 4, 8, (2, 13), (42, 53))            # 11 x 11: kept, margin 1
    paint(inst, sem, 6, 15, (18, 35), (40, 59))          # partly overwritten by 300
    paint(inst, sem, 300, 11, (20, 33), (28, 45))        # an id above 255
    paint(inst, sem, 5, 9, (36, 48), (50, 64))           # touches the right and the bottom border: clipped
    return (*colour_and_depth(rng, W, H), inst, sem)


def noise_frame():
    """150 x 70 (no multiple of any tile): some 40 ids on a coarse random grid, so that several share every tile; classes drawn per
    id, some from the background list."""
    W, H = 150, 70
    rng = np.random.default_rng(202)
    labels = np.concatenate([[0], rng.choice(np.arange(1, 600), 39, replace=False)]).astype(np.uint16)
    classes = rng.choice(np.array([3, 7, 11, 20, 26, 44, 61, 80, 31, 40, 93, 97]), labels.size).astype(np.uint16)
    cells = rng.integers(0, labels.size, (-(-H // 6), -(-W // 11)))
    idx = np.repeat(np.repeat(cells, 6, axis=0), 11, axis=1)[:H, :W]
    inst, sem = labels[idx], classes[idx]
    return (*colour_and_depth(rng, W, H), inst, sem)


def main():
    ref_dataset = import_reference_dataset()
    tmp = tempfile.mkdtemp()
    np.savetxt(os.path.join(tmp, "traj_w_c.txt"), np.eye(4).reshape(1, 16))
    for name, frame, imap in (("rects", rects_frame, False), ("noise", noise_frame, False), ("imap", rects_frame, True)):
        rgb, depth, inst, sem = frame()
        FILES.clear()
        FILES.update(rgb=rgb[..., ::-1], depth=depth, semantic_instance=inst, semantic_class=sem)
        cfg = types.SimpleNamespace(imap_mode=imap, dataset_dir=tmp, depth_scale=DEPTH_SCALE, max_depth=MAX_DEPTH)
        ds = ref_dataset.Replica(cfg)
        s = ds[0]
        ids = sorted(int(k) for k in s["bbox_dict"])
        boxes = np.asarray([[int(x) for x in s["bbox_dict"][k]] for k in ids], np.int32).reshape(-1, 4)
        out = dict(rgb=rgb, depth=depth, inst=inst, sem=sem, depth_scale=np.float64(DEPTH_SCALE), max_depth=np.float64(MAX_DEPTH),
                   bbox_scale=np.float64(ds.bbox_scale), min_box=np.int32(10), background=np.asarray(ds.background_cls_list, np.int32),
                   imap=np.bool_(imap), ref_image=np.asarray(s["image"], np.uint8), ref_depth=np.asarray(s["depth"], np.float32),
                   ref_obj=np.asarray(s["obj"], np.int32), ref_bbox_ids=np.asarray(ids, np.int32), ref_bbox=boxes)
        # the checker must already agree (this is the pin)
        o = io.ingest(rgb, depth, None if imap else inst, None if imap else sem, DEPTH_SCALE, MAX_DEPTH, ds.background_cls_list, ds.bbox_scale, 10)
        assert np.array_equal(o["inst"], out["ref_obj"]) and np.array_equal(o["rgbx"][..., :3], out["ref_image"])
        assert np.array_equal(o["depth"].view(np.uint32), out["ref_depth"].view(np.uint32))
        bd = io.bbox_dict(o["rows"])
        assert sorted(bd) == ids and all(bd[k] == list(b) for k, b in zip(ids, boxes.tolist())), (bd, ids, boxes)
        path = os.path.join(HERE, f"ingest_{name}.npz")
        np.savez_compressed(path, **out)
        st = {io.KEPT: 0, io.BACKGROUND: 0, io.SMALL: 0, io.ZERO_MARGIN: 0, io.ABSENT: 0}
        for r in o["rows"]:
            st[int(r[1])] += 1
        print(f"{name:6s} {rgb.shape[1]} x {rgb.shape[0]}: {len(o['rows'])} ids, kept {st[io.KEPT]}, background {st[io.BACKGROUND]}, "
              f"small {st[io.SMALL]}, boxes {len(ids)} -> {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
