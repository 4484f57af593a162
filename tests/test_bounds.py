"""Object bounds, CPU tier: the oriented-box search of vmap_amd/bounds.py on the numpy backend (analytic clouds, the conditions every
returned box meets, the None cases, batches against single calls, the synthetic keyframe scene) and the argument checks of the new C
functions.  No device: the HIP kernels are covered by tests/test_gpu_bounds.py.

Bounds used here, all derived:
- theta = sqrt(3) * FINAL_STEP_DEG: the search ends on a grid of rotation vectors with that step per component, so a frame within the
  grid's reach is off by at most sqrt(3) steps; a box of extents e measured in a frame off by theta grows by at most
  prod_i (1 + theta (e_j + e_k) / e_i) (bounds_oracle.volume_inflation);
- tol = 2^-20 max |p - c|: a few float32 roundings of a three-term dot product; an extent is two such ends (_extent_slack takes
  max |p - c| as sqrt(3) times the largest coordinate of the cloud about the middle of its range)."""
import ctypes
import math

import numpy as np
import pytest

import bounds_oracle as bo
from vmap_amd import _lib, bounds
from vmap_amd.evaluation import principal_axes_box

THETA = math.sqrt(3.0) * math.radians(bounds.FINAL_STEP_DEG)

# name -> (cloud maker, extents of the known smallest box)
CLOUDS = {
    "box_1x2x5": (lambda n, rng, R, c: bo.box_cloud((1, 2, 5), n, rng, R, c), (1, 2, 5)),
    "box_1x1x10": (lambda n, rng, R, c: bo.box_cloud((1, 1, 10), n, rng, R, c), (1, 1, 10)),
    "cube": (lambda n, rng, R, c: bo.box_cloud((1, 1, 1), n, rng, R, c), (1, 1, 1)),
    "slab_0.1x2x3": (lambda n, rng, R, c: bo.box_cloud((0.1, 2, 3), n, rng, R, c), (0.1, 2, 3)),
    "l_shape": (bo.l_shape_cloud, (1, 3, 3)),
    "tetrahedron": (bo.tetrahedron_cloud, (1, 1, 1)),
}


def _make(name, seed, n=3000):
    rng = np.random.default_rng(seed)
    R = bo.random_rotations(rng, 1)[0]
    c = rng.uniform(-2, 2, 3)
    maker, extent = CLOUDS[name]
    return maker(n, rng, R, c).astype(np.float32), np.asarray(extent, np.float64)


def _extent_slack(points, extent):
    """prod_i (1 + 2 tol / e_i): how far float32 rounding of the six projections can move a volume."""
    p = np.asarray(points, np.float64)
    tol = 2.0 ** -20 * np.abs(p - 0.5 * (p.min(0) + p.max(0))).max() * math.sqrt(3.0)
    return float(np.prod(1 + 2 * tol / np.asarray(extent, np.float64)))


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_search_on_analytic_clouds(name):
    pts, extent = _make(name, seed=sorted(CLOUDS).index(name))
    (box,), info = bounds.oriented_bounds(pts, backend="numpy", return_info=True)
    assert box is not None
    true = float(np.prod(extent))
    found = float(info["volume"][0])
    slack = _extent_slack(pts, extent)
    upper = true * bo.volume_inflation(extent, THETA)
    print(f"{name}: found / true = {found / true:.6f}, bound {upper / true:.6f}")
    assert found >= true / slack, (found, true)
    assert found <= upper * slack, (found / true, upper / true)
    # by construction: never worse than the coarse set's best, the axis-aligned box, the principal-axes box
    p64 = pts.astype(np.float64)
    aabb = float(np.prod(p64.max(0) - p64.min(0)))
    pab = float(np.prod(principal_axes_box(pts).extent))
    assert found <= info["coarse_volume"][0]
    assert found <= aabb * slack, (found, aabb)
    assert found <= pab * slack, (found, pab)
    assert bo.box_violations(box, pts) == []


def test_tetrahedron_beats_a_coarse_exhaustive_grid():
    pts, _ = _make("tetrahedron", seed=11, n=400)
    _, info = bounds.oriented_bounds(pts, backend="numpy", return_info=True)
    grid = bo.exhaustive_search(pts, step_deg=5.0)
    assert info["volume"][0] <= grid * (1 + 1e-6), (info["volume"][0], grid)


def test_none_cases_and_the_smallest_cloud():
    rng = np.random.default_rng(5)
    three = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
    assert bounds.oriented_bounds(three, backend="numpy") == [None]
    assert bounds.oriented_bounds(np.zeros((0, 3), np.float32), backend="numpy") == [None]
    flat = np.concatenate([rng.uniform(-1, 1, (500, 2)), np.zeros((500, 1))], 1)
    assert bounds.oriented_bounds(flat.astype(np.float32), backend="numpy") == [None]
    tilted = (flat @ bo.rotation((1, -1, 0.5), 0.7).T).astype(np.float32)
    assert bounds.oriented_bounds(tilted, backend="numpy") == [None]
    tet = (np.array([[0, 0, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1]], np.float64) @ bo.rotation((1, 1, 0), 0.3).T).astype(np.float32)
    (box,) = bounds.oriented_bounds(tet, backend="numpy")
    assert box is not None and bo.box_violations(box, tet) == []
    assert np.prod(box.extent) <= 1.0 * bo.volume_inflation((1, 1, 1), THETA) * _extent_slack(tet, (1, 1, 1))


def test_a_batch_equals_the_single_calls_bit_for_bit():
    parts = [_make("box_1x2x5", 1, 700)[0], np.zeros((0, 3), np.float32), _make("cube", 2, 300)[0] * 0.05,
             _make("cube", 3, 3)[0][:3], _make("tetrahedron", 4, 900)[0] * 40.0]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    batch = bounds.oriented_bounds(np.concatenate(parts), offsets, backend="numpy")
    assert [b is None for b in batch] == [False, True, False, True, False]
    for p, b in zip(parts, batch):
        (single,) = bounds.oriented_bounds(p, backend="numpy")
        assert (single is None) == (b is None)
        if b is not None:
            for k in ("center", "R", "extent"):
                np.testing.assert_array_equal(getattr(single, k), getattr(b, k))
            assert bo.box_violations(b, p) == []
    assert np.all(batch[2].extent >= bounds.MIN_EXTENT)          # the 5 cm cube: extents clamped as the reference does
    assert batch[2].extent[0] == bounds.MIN_EXTENT


def test_coarse_set_and_shipped_parameters():
    R = bounds.coarse_rotations()
    assert R.shape == (bounds.COARSE_DIRECTIONS * bounds.COARSE_ANGLES, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.all(np.linalg.det(R) > 0)
    assert R[:, 0, 2].min() > 0                                        # first axes on the upper hemisphere
    assert bounds.GRID % 2 == 1 and bounds.SEEDS * bounds.GRID ** 3 <= 1024
    assert f"{bounds.FINAL_STEP_DEG:.4f}" in bounds.__doc__ and f"{bounds.DELTA0_DEG:.4f}" in bounds.__doc__


def scene_conditions(scene, boxes, clouds, label):
    """Item 8 of the issue for every object of the scene: containment and the box conditions on the cloud, each sorted extent within
    two pixel footprints of the true box's, the volume below the true volume times the inflation bound."""
    fp = scene.footprint()
    msgs = []
    for b, box, pts in zip(scene.boxes, boxes, clouds):
        assert box is not None, label
        assert bo.box_violations(box, pts) == [], label
        true = np.sort(b["extent"])
        got = np.asarray(box.extent)
        msgs.append(f"{label} id {b['id']}: extents {got} vs {true}, volume ratio {np.prod(got) / np.prod(true):.5f}")
        assert np.abs(got - true).max() <= 2 * fp, msgs[-1]
        assert np.prod(got) <= np.prod(true) * bo.volume_inflation(true, THETA) * _extent_slack(pts, true), msgs[-1]
    return msgs


def test_scene_through_the_numpy_backend():
    scene = bo.Scene()
    clouds = [scene.cloud(b["id"])[0].astype(np.float32)[::8] for b in scene.boxes]        # thinned: the CPU tier's time
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    boxes = bounds.oriented_bounds(np.concatenate(clouds), offsets, backend="numpy")
    for m in scene_conditions(scene, boxes, clouds, "numpy"):
        print(m)


def test_extents_backend_matches_the_checker():
    rng = np.random.default_rng(9)
    pts = (rng.standard_normal((1234, 3)) * (1.0, 3.0, 0.2) + 5.0).astype(np.float32)
    rot = bo.random_rotations(rng, 37).astype(np.float32)
    c = np.array([[5.0, 5.0, 5.0]], np.float32)
    lo, hi = bounds.extents(pts, rot, center=c, backend="numpy")
    lo64, hi64, slo, shi = bo.extents64(pts, rot, c[0])
    assert np.all(np.abs(lo[0].numpy() - lo64) <= 2.0 ** -22 * slo) and np.all(np.abs(hi[0].numpy() - hi64) <= 2.0 ** -22 * shi)


def test_new_functions_check_their_arguments_without_a_device():
    lib = _lib.load()
    nb = ctypes.c_size_t()
    assert lib.vmapstep_unproject_workspace_bytes(4, 2, 160, 120, ctypes.byref(nb)) == 0 and nb.value >= 4 * 19 * 8 + 2 * 24
    assert lib.vmapstep_unproject_workspace_bytes(4, 2, 160, 120, None) == -1
    assert lib.vmapstep_unproject_workspace_bytes(-1, 2, 160, 120, ctypes.byref(nb)) == -1
    assert lib.vmapstep_unproject_workspace_bytes(4, 0, 160, 120, ctypes.byref(nb)) == -1
    assert lib.vmapstep_unproject_workspace_bytes(4, 2, 0, 120, ctypes.byref(nb)) == -1
    k4 = (ctypes.c_float * 4)(150, 150, 80, 60)
    first = (ctypes.c_int32 * 3)(0, 2, 4)
    fake = 256                                                       # a non-null pointer nothing dereferences: every call below is refused first
    head = (fake, fake, fake, 10, 160, 120, k4, fake, fake, first, 2, 4)
    assert lib.vmapstep_unproject_count(None, *head[1:], fake, fake, fake, nb.value, None) == -1
    assert b"null" in lib.vmapstep_last_error()
    assert lib.vmapstep_unproject_count(*head, None, fake, fake, nb.value, None) == -1
    assert lib.vmapstep_unproject_count(*head[:4], -160, *head[5:], fake, fake, fake, nb.value, None) == -1
    bad_first = (ctypes.c_int32 * 3)(0, 3, 2)
    assert lib.vmapstep_unproject_count(*head[:9], bad_first, 2, 4, fake, fake, fake, nb.value, None) == -1
    assert b"first_pair" in lib.vmapstep_last_error()
    assert lib.vmapstep_unproject_count(*head, fake, fake, None, nb.value, None) == -3           # workspace
    assert lib.vmapstep_unproject_count(*head, fake, fake, fake, nb.value - 1, None) == -3
    assert lib.vmapstep_unproject_count(*head, fake, fake, fake + 1, nb.value, None) == -3        # misaligned
    assert lib.vmapstep_unproject_emit(*head, None, 5, fake, nb.value, None) == -1
    assert lib.vmapstep_unproject_emit(*head, fake, -1, fake, nb.value, None) == -1
    assert lib.vmapstep_unproject_emit(*head, None, 0, fake, nb.value, None) == 0                # nothing to write: accepted, nothing enqueued

    off = (ctypes.c_int64 * 3)(0, 5, 9)
    ext = lambda *a: lib.vmapstep_obb_extents(*a)
    assert ext(fake, 9, fake, off, 2, None, fake, 0, 0, 0, fake, fake, None) == -1 and b"K=0" in lib.vmapstep_last_error()
    assert ext(fake, 9, fake, off, 0, None, fake, 0, 4, 0, fake, fake, None) == -1
    assert ext(fake, -1, fake, off, 2, None, fake, 0, 4, 0, fake, fake, None) == -1
    assert ext(fake, 8, fake, off, 2, None, fake, 0, 4, 0, fake, fake, None) == -1 and b"past the array" in lib.vmapstep_last_error()
    assert ext(fake, 9, fake, None, 2, None, fake, 0, 4, 0, fake, fake, None) == -1
    assert ext(None, 9, fake, off, 2, None, fake, 0, 4, 0, fake, fake, None) == -1
    assert ext(fake, 9, fake, off, 2, None, None, 0, 4, 0, fake, fake, None) == -1
    assert ext(fake, 9, fake, off, 2, None, fake, 0, 4, 0, None, fake, None) == -1
    assert ext(fake, 9, fake, off, 2, None, fake, 35, 4, 0, fake, fake, None) == -1 and b"set_stride" in lib.vmapstep_last_error()
    assert ext(fake, 9, fake, off, 2, None, fake, 0, 4, -1, fake, fake, None) == -1 and b"point_chunks" in lib.vmapstep_last_error()
    assert ext(fake, 9, fake, off, 2, None, fake, 0, 2 ** 30, 0, fake, fake, None) == -1
    assert lib.vmapstep_cloud_moments(fake, 9, fake, off, 2, None, None, None) == -1
    assert lib.vmapstep_cloud_moments(fake, 9, fake, off, 0, None, fake, None) == -1
    dec = (ctypes.c_int64 * 3)(0, 5, 4)
    assert lib.vmapstep_cloud_moments(fake, 9, fake, dec, 2, None, fake, None) == -1 and b"decrease" in lib.vmapstep_last_error()
