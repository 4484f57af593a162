"""The frames of the instance-filter tests (tests/test_filter.py, tests/test_gpu_filter.py): one 75 x 53 frame (W x H, a multiple of
no tile dimension) that holds every case the contract names, and a three-frame sequence with a moving pose.  Ids below are SHIFTED ids
(raw = id - id_shift); min_pixels is 30 so that a frame this small exercises every branch."""
from __future__ import annotations

import numpy as np

W, H = 75, 53
MAX_IDS = 64
INTRINSICS = (60.0, 60.0, 37.0, 26.0)
BACKGROUND = (1, 3)
SETTINGS = dict(depth_scale=1.0 / 1000.0, max_depth=8.0, background=BACKGROUND, min_pixels=30, min_points=10, voxel_size=0.02, max_ids=MAX_IDS)

ID_NEW, ID_CORNER, ID_STRIP, ID_FILL, ID_LEFT, ID_RIGHT, ID_FEW, ID_RIM, ID_LATE, ID_LAST = 2, 3, 4, 5, 6, 7, 8, 9, 10, MAX_IDS - 1


def class_of(idv):
    return 1 if idv == ID_FILL else 50 + idv


def base_frame():
    """(ids int64 [H, W] shifted, sem, raw depth uint16): a curved surface about 2 m away, so that no cloud is flat."""
    v, u = np.mgrid[0:H, 0:W]
    ids = np.full((H, W), ID_FILL, np.int64)                  # a background-class instance everywhere else
    ids[2:25, 28:51] = ID_NEW                                 # 23 x 23: erodes to 11 x 11 at radius 6 ...
    ids[4, 30] = ID_FILL                                      # ... less what a one-pixel hole takes
    ids[0:16, 0:16] = ID_CORNER                               # on the top-left corner: the window is clipped to the image
    ids[17:27, 0:13] = ID_LAST                                # the last id of the table; too low to survive radius 6
    ids[28:51, 2:11] = ID_STRIP                               # 9 wide, off the border: erodes to nothing at radius 6
    ids[28:51, 14:34] = ID_LEFT                               # two blobs sharing an edge
    ids[28:51, 34:54] = ID_RIGHT
    ids[28:51, 56:73] = ID_FEW                                # 10 valid pixels
    ids[2:25, 52:75] = ID_RIM                                 # on the right border; its eroded region has depth 0, its rim is valid
    ids[51:53, :] = 0                                         # a raw id that shifts to 0
    depth = (2000.0 + 300.0 * np.sin(u / 5.0) + 200.0 * np.cos(v / 4.0)).astype(np.uint16)
    few = ids == ID_FEW
    depth[few] = 0
    depth[30, 58:68] = 2100                                   # exactly min_points valid pixels
    depth[6:21, 56:75] = 0                                    # covers the eroded region of ID_RIM at radius 6 (rows 8..18, cols 58..74)
    depth[3, 29] = 65000                                      # beyond max_depth
    depth[10, 45] = 0
    sem = np.vectorize(class_of)(ids).astype(np.int64)
    return ids, sem, depth


def typed(ids, sem, depth, wide):
    """The inputs as a caller holds them: u16 everything with id_shift 0, or float32 depth and int32 labels with id_shift 1 (raw -1
    shifts to 0) and a NaN where the 16-bit frame has a 0."""
    if not wide:
        return depth.astype(np.uint16), ids.astype(np.uint16), sem.astype(np.uint16), 0
    d = depth.astype(np.float32)
    d[10, 45] = np.nan
    return d, (ids - 1).astype(np.int32), sem.astype(np.int32), 1


def pose(tx=0.0, ty=0.0, tz=0.0, yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    T[:3, 3] = (tx, ty, tz)
    return T


def sequence():
    """Three frames [(ids, sem, depth, t_wc)]: frame 1 registers; in frame 2 the camera has moved, ID_CORNER lies 1.5 m deeper (all of
    it outside its box) and ID_LATE appears where ID_FEW was; frame 3 moves again."""
    ids, sem, depth = base_frame()
    ids2, depth2 = ids.copy(), depth.copy()
    depth2[ids == ID_CORNER] += 1500
    late = ids == ID_FEW
    ids2[late] = ID_LATE
    v, u = np.mgrid[0:H, 0:W]
    depth2[late] = (2200.0 + 250.0 * np.sin(u / 3.0) + 150.0 * np.cos(v / 5.0)).astype(np.uint16)[late]
    sem2 = np.vectorize(class_of)(ids2).astype(np.int64)
    return [(ids, sem, depth, pose()), (ids2, sem2, depth2, pose(0.05, -0.02, 0.03, 0.02)), (ids2, sem2, depth2, pose(0.12, 0.0, -0.05, -0.03))]
