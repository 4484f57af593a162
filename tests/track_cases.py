"""The frames of the instance-tracker tests (tests/test_track.py, tests/test_gpu_track.py): 75 x 53 frames (W x H, a multiple of no
tile dimension), thresholds small enough for a dozen objects per frame.  A frame is (rows int64 [H, W], det_classes, raw depth uint16,
t_wc); rows are detection ROWS (raw = row - det_shift), row 0 = no detection.  Pixel spacing at 2 m is 33 mm, a voxel 40 mm."""
from __future__ import annotations

import numpy as np

from filter_cases import pose  # noqa: F401

W, H = 75, 53
INTRINSICS = (60.0, 60.0, 37.0, 26.0)
BACKGROUND = (1, 3)
SETTINGS = dict(depth_scale=1.0 / 1000.0, max_depth=8.0, background=BACKGROUND, match_ratio=0.5, min_pixels=20, min_points=10, erode_radius=1,
                voxel_size=0.04, min_extent=0.05, max_det=32, max_pairs=256, max_ids=64)

# the objects of the main sequence: name -> (row slice, column slice, class)
OBJECTS = dict(A=((2, 16), (2, 18), 50), B=((2, 16), (20, 36), 50), C=((2, 16), (38, 54), 51), BG=((2, 16), (56, 73), 3),
               THIN=((18, 20), (2, 30), 54), FEW=((24, 38), (2, 18), 52), TINY=((24, 38), (20, 36), 52), D=((24, 38), (38, 54), 51),
               E=((40, 52), (2, 26), 53))
ORDER_1 = ("A", "B", "C", "BG", "THIN", "FEW", "TINY", "D", "E")                  # detection rows 1 .. 9 of frame 1
ORDER_2 = ("E", "BG", "D", "A", "FEW", "C", "THIN", "B")                          # frame 2: permuted, TINY gone
# frame 1 on an empty state: A, B, C -> ids 1, 2, 3; TINY takes id 4 and loses it (NEW_NO_BOX); D -> 5, E -> 6
IDS = dict(A=1, B=2, C=3, D=5, E=6)


def surface():
    """raw depth uint16: a curved surface about 2 m away, so that no cloud is flat"""
    v, u = np.mgrid[0:H, 0:W]
    return (2000.0 + 300.0 * np.sin(u / 5.0) + 200.0 * np.cos(v / 4.0)).astype(np.uint16)


def paint(rows, region, d):
    (r0, r1), (c0, c1) = region[0], region[1]
    rows[r0:r1, c0:c1] = d


def layout(order):
    """(rows, det_classes, depth) of the named objects as detection rows 1, 2, ... in `order`."""
    rows = np.zeros((H, W), np.int64)
    classes = [0]
    depth = surface()
    for d, name in enumerate(order, 1):
        paint(rows, OBJECTS[name], d)
        classes.append(OBJECTS[name][2])
    if "FEW" in order:                                        # depth 0 but for exactly min_points pixels of its eroded mask
        (r0, r1), (c0, c1), _ = OBJECTS["FEW"]
        depth[r0:r1, c0:c1] = 0
        depth[30, 5:15] = 2100
    if "TINY" in order:                                       # 0.1 m away: its eroded mask falls into two voxels, so its cloud has no box
        (r0, r1), (c0, c1), _ = OBJECTS["TINY"]
        depth[r0:r1, c0:c1] = 100
    depth[3, 4] = 65000                                       # beyond max_depth
    depth[10, 45] = 0
    return rows, classes, depth


def main_sequence():
    """Frame 1: every non-match status on an empty state.  Frame 2: the same objects under permuted rows from a moved pose.  Frame 3,
    moved again: C's place under another class (NEW), E's place inside a detection three times its size (below the ratio: NEW), A as
    two detections (both MERGED into A's id), B as it was."""
    f1 = layout(ORDER_1) + (pose(),)
    f2 = layout(ORDER_2) + (pose(0.05, -0.02, 0.03, 0.02),)
    rows = np.zeros((H, W), np.int64)
    depth = surface()
    classes = [0, 77, 53, 50, 50, 50]
    paint(rows, OBJECTS["C"], 1)                              # class mismatch
    paint(rows, ((40, 52), (2, 72)), 2)                       # below threshold
    paint(rows, ((2, 16), (2, 10)), 3)                        # shared match, left half of A
    paint(rows, ((2, 16), (10, 18)), 4)                       # shared match, right half of A
    paint(rows, OBJECTS["B"], 5)
    f3 = (rows, classes, depth, pose(0.08, 0.0, -0.02, -0.01))
    return [f1, f2, f3]


def edge_frame():
    """Frame 1 without TINY, whose few voxels depend on where the pose puts it: for poses that lay the end of the key grid across C and
    D (x = 32768 voxels; the camera's x = 0.3 m runs through the middle of both)."""
    return layout(tuple(n for n in ORDER_1 if n != "TINY"))


def overlap_sequence():
    """Two instances of one class whose boxes overlap, then a detection inside both: frame 1 registers columns 2..17 (id 1); frame 2's
    detection spans columns 10..39, less than half of it inside id 1's box, so it becomes id 2; frame 3's spans columns 6..23 - more
    than half inside either box, and more of it inside id 2's.  The lower id wins."""
    frames = []
    for c0, c1 in ((2, 18), (10, 40), (6, 24)):
        rows = np.zeros((H, W), np.int64)
        paint(rows, ((2, 16), (c0, c1)), 1)
        frames.append((rows, [0, 50], surface(), pose()))
    return frames


OVERFLOW_OBJECTS = 10


def overflow_sequence(pair_slots):
    """Ten instances of one class over two frames, then a frame whose first tile (64 x 16) holds twelve one-pixel-high detections of
    that class on the image rows 0, 4 and 8 - rows that one wave of the workgroup owns, so that the order in which the pairs reach
    the LDS table is fixed: 12 x 10 = 120 pairs, of which the first `pair_slots` fill the table; the detections of row 8 lie inside
    registered boxes, and none of their pairs finds a slot."""
    assert 8 * OVERFLOW_OBJECTS >= pair_slots + 4
    frames = []
    for r0 in (2, 16):
        rows = np.zeros((H, W), np.int64)
        for k in range(5):
            paint(rows, ((r0, r0 + 12), (1 + 15 * k, 14 + 15 * k)), k + 1)
        frames.append((rows, [0] + [60] * 5, surface(), pose()))
    rows = np.zeros((H, W), np.int64)
    for k in range(12):
        y, c0 = 4 * (k // 4), 16 * (k % 4)
        rows[y, c0:c0 + 16] = k + 1
    frames.append((rows, [0] + [60] * 12, surface(), pose()))
    return frames


def typed(rows, depth, wide):
    """The inputs as a caller holds them: u16 everything with det_shift 0, or float32 depth and an int32 label image with det_shift 1
    (row 0 is raw -1) and a NaN where the 16-bit frame has a 0.  -> (depth, det, det_shift)"""
    if not wide:
        return depth.astype(np.uint16), rows.astype(np.uint16), 0
    d = depth.astype(np.float32)
    d[10, 45] = np.nan
    return d, (rows - 1).astype(np.int32), 1
