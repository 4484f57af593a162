"""CPU tier: the mesh-extraction, mesh-evaluation and object-bounds kernel SOURCE (vmap_amd/csrc/mesh_kernels.h, eval_kernels.h,
bounds_kernels.h, and the scans of scan_ops.h they share) executed lane by lane on the SIMT executor of tests/sim, against the float64
numpy checkers the GPU tier uses (mesh_oracle, eval_oracle, bounds_oracle).  Workspace layouts and launch plans are the product's own
(launch_geometry.h); every output and workspace is poisoned and guarded by the wrappers of tests/simlib.py.

Every case runs under the executor's three schedules (0 round-robin, 1 / 2 wave-greedy forward / reverse) and must give identical
bytes: a wave running ahead of the others through a missing barrier changes a result under 1 or 2.  Integers, orders and bit patterns
are compared exactly; float32-vs-float64 tolerances are those of the GPU-tier test of the same operation."""
import numpy as np
import pytest

import bounds_oracle as bo
import eval_oracle as eo
import mesh_oracle as mo
import simlib
from conftest import load_golden
from geom_checks import check_clip_against_oracle, check_mesh_against_oracle, check_nn, nn_exempt_share, rotation_qr, whole_triangle_case
from philox_ref import M32, philox4x32_10, surface_randoms

SCHEDULES = (0, 1, 2)


def _same(a, b, where=""):
    if isinstance(a, dict):
        for k in a:
            _same(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (tuple, list)):
        for j, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{j}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"schedules disagree on {where}"
    else:
        assert a == b, f"schedules disagree on {where}"


def run3(fn):
    """fn() under the three schedules: identical bytes required; returns the round-robin result.  Each run is made in a child process
    (simlib.isolated): a kernel that faults on the host - a division by a zero chunk count, a read far outside a buffer - fails the
    one test that ran it and the rest of the tier goes on."""
    outs = []
    try:
        for s in SCHEDULES:
            simlib.set_schedule(s)
            outs.append(simlib.isolated(fn))
    finally:
        simlib.set_schedule(0)
    for s, o in zip(SCHEDULES[1:], outs[1:]):
        _same(outs[0], o, f"schedule {s}")
    return outs[0]


# ---- the executor's own test: the wave-greedy schedules see a missing barrier ------------------------------------------------------

def test_wave_greedy_schedules_see_two_scans_through_one_wsum():
    """tests/sim/sim_hazard.cpp: two wg_exclusive_scan calls in a row.  Through ONE wsum with no barrier between them (what scan_ops.h's
    barrier contract forbids) a wave that is past the first scan's barrier overwrites sums other waves have not read yet.  Round-robin
    lets no wave run ahead and cannot see it; both wave-greedy orders must.  The twin with an array per scan is right under all three."""
    rng = np.random.default_rng(0)
    x, y = rng.integers(0, 9, 512), rng.integers(0, 9, 512)
    want = (np.cumsum(x) - x, np.cumsum(y) - y, np.tile([x.sum(), y.sum()], (512, 1)))
    wrong = {}
    try:
        for s in SCHEDULES:
            simlib.set_schedule(s)
            ex, ey, tot = simlib.sim_scan_hazard(0, x, y)
            assert (ex == want[0]).all() and (ey == want[1]).all() and (tot == want[2]).all(), f"the correct kernel, schedule {s}"
            ex, ey, tot = simlib.sim_scan_hazard(1, x, y)
            wrong[s] = int((ex != want[0]).sum() + (ey != want[1]).sum() + (tot != want[2]).any(1).sum())
    finally:
        simlib.set_schedule(0)
    assert wrong[0] == 0          # the reason the second schedule exists: if round-robin ever sees this, say so here
    assert wrong[1] > 0 and wrong[2] > 0, wrong


def test_step_kernels_give_the_same_bytes_under_every_schedule():
    """The wave-greedy schedules are compatible with the kernels the executor ran before them: the fused step (prep, main, finalize)
    of the 'ragged' parity case, loss, renders and every gradient, bit for bit."""
    import cases
    c = cases.build_case("ragged")
    run3(lambda: {k: np.asarray(v) for k, v in simlib.sim_step(c).items()})


# ---- mesh extraction ---------------------------------------------------------------------------------------------------------------

MESH_FIXTURES = ("sphere", "blob", "noncubic", "noise", "exact", "tiny")


def _block_totals(vol, level=0.5):
    """(vertices, faces) of every workgroup of 256 grid points, from the volume alone: int64 [nblk, 2]."""
    up = vol > level
    nx, ny, nz = vol.shape
    nv = np.zeros(vol.shape, np.int64)
    nv[:-1] += up[1:] != up[:-1]
    nv[:, :-1] += up[:, 1:] != up[:, :-1]
    nv[:, :, :-1] += up[:, :, 1:] != up[:, :, :-1]
    u = up.astype(np.int64)
    c = (u[:-1, :-1, :-1] | u[:-1, :-1, 1:] << 1 | u[:-1, 1:, 1:] << 2 | u[:-1, 1:, :-1] << 3 | u[1:, :-1, :-1] << 4 | u[1:, :-1, 1:] << 5 |
         u[1:, 1:, 1:] << 6 | u[1:, 1:, :-1] << 7)
    nf = np.zeros(vol.shape, np.int64)
    nf[:-1, :-1, :-1] = (mo.triangle_table()[:, ::3] >= 0).sum(1)[c]
    pad = (-vol.size) % 256
    per = lambda a: np.concatenate([a.ravel(), np.zeros(pad, np.int64)]).reshape(-1, 256).sum(1)      # noqa: E731
    return np.stack([per(nv), per(nf)], 1)


def _check_mesh(vol, level=0.5, affine=None, normals=True):
    m = run3(lambda: simlib.sim_mesh(vol, level, affine, normals))
    v, f, _, _ = mo.marching_cubes(vol, level, affine)
    assert m["counts"].tolist() == [len(v), len(f)]
    tot = _block_totals(vol, level)
    np.testing.assert_array_equal(m["blk"], np.cumsum(tot, 0) - tot)          # the exclusive prefix mesh_scan leaves, both columns
    if len(v):
        check_mesh_against_oracle(vol, m["vertices"], m["faces"], m["normals"], affine, level)
    return m, tot


@pytest.mark.parametrize("name", MESH_FIXTURES)
def test_sim_mesh_fixtures_equal_oracle(name):
    _check_mesh(load_golden(f"mesh_{name}")["volume"])


@pytest.mark.parametrize("shape", [(2, 2, 2), (5, 6, 7), (7, 9, 11), (16, 16, 1 + 16), (3, 2, 129)], ids=str)
def test_sim_mesh_small_and_ragged_volumes(shape):
    """Fewer points than one workgroup (8, 210), counts that are no multiple of 256 (693, 4352 + 0, 774)."""
    rng = np.random.default_rng(sum(shape))
    _check_mesh(rng.uniform(0, 1, shape).astype(np.float32))


@pytest.mark.slow
@pytest.mark.parametrize("shape,edges", [((65, 65, 65), (1024,)), ((81, 81, 81), (1024, 2048))], ids=["1073 blocks", "2076 blocks"])
def test_sim_mesh_scan_past_its_chunks(shape, edges):
    """A noise volume of more than 1024 / 2048 workgroups: mesh_scan's running carry crosses one / two chunk edges with both packed
    columns (vertices low, faces high) non-zero and different in every wave."""
    rng = np.random.default_rng(shape[0])
    vol = rng.uniform(0, 1, shape).astype(np.float32)
    m, tot = _check_mesh(vol, normals=False)
    for e in edges:
        assert (m["blk"][e] > 0).all() and (tot[e - 1] > 0).all() and m["blk"][e][0] != m["blk"][e][1]


def test_sim_mesh_without_a_crossing():
    vol = np.full((9, 8, 7), 0.25, np.float32)
    for level in (0.5, 0.25):                     # strictly above the level counts: a volume AT the level has no crossing either
        m = run3(lambda: simlib.sim_mesh(vol, level))
        assert m["counts"].tolist() == [0, 0] and not m["blk"].any() and not m["emask"].any()


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("affine", [None, [[0.0, 0.05, 0.01, 1.0], [-0.04, 0.0, 0.02, -2.0], [0.01, 0.0, 0.07, 0.5]]], ids=["index", "affine"])
def test_sim_mesh_affine_and_normals(affine, normals):
    vol = load_golden("mesh_noncubic")["volume"]
    _check_mesh(vol, 0.5, affine, normals)
    _check_mesh(vol, 0.3, affine, normals)


def test_sim_mesh_capacities_below_the_totals():
    """Nothing at or past n_vertices / n_faces is written (the buffers END there, followed by guard bytes), and what is written is the
    prefix of the full result, bit for bit."""
    vol = load_golden("mesh_blob")["volume"]
    A = [[0.0, 0.05, 0.01, 1.0], [-0.04, 0.0, 0.02, -2.0], [0.01, 0.0, 0.07, 0.5]]
    full = run3(lambda: simlib.sim_mesh(vol, 0.5, A))
    nv, nf = full["counts"]
    assert nv > 600 and nf > 600
    for cv, cf in ((nv // 2, nf // 3), (1, 1), (nv - 1, nf - 1), (0, 0), (nv, 0)):
        m = run3(lambda: simlib.sim_mesh(vol, 0.5, A, True, cv, cf))
        assert m["counts"].tolist() == [nv, nf]
        assert m["vertices"].tobytes() == full["vertices"][:cv].tobytes()
        assert m["normals"].tobytes() == full["normals"][:cv].tobytes()
        assert m["faces"].tobytes() == full["faces"][:cf].tobytes()


def test_sim_mesh_grid_points():
    """A (i, j, k) + b over the grid, C order; against float64 within a few float32 roundings of the terms' magnitudes."""
    A = np.array([[0.03, 0.001, -0.002, -1.0], [0.0, 0.04, 0.003, 0.7], [-0.001, 0.002, 0.05, 2.5]], np.float32)
    shape = (5, 19, 13)                                    # 1235 points: a partial last workgroup
    got = run3(lambda: simlib.sim_mesh_grid_points(shape, A))
    ijk = np.stack(np.unravel_index(np.arange(int(np.prod(shape))), shape), -1).astype(np.float64)
    A64 = A.astype(np.float64)
    want = ijk @ A64[:, :3].T + A64[:, 3]
    mag = np.abs(ijk) @ np.abs(A64[:, :3]).T + np.abs(A64[:, 3])
    assert (np.abs(got - want) <= 4 * 2.0 ** -24 * mag).all()          # three fused multiply-adds: three roundings, and the output's


# ---- nearest neighbours ------------------------------------------------------------------------------------------------------------

TILE, QB, NNWG = 512, 2048, 256            # kNnTile, kNnQB, kNnWG (csrc/launch_geometry.h)


def _cloud(rng, n, offset=0.0):
    return (rng.uniform(-1, 1, (n, 3)) + offset).astype(np.float32)


def _nn3(q, r, **kw):
    return run3(lambda: {k: v for k, v in simlib.sim_nn(q, r, **kw).items() if k != "plan"})


# queries around kNnWG and kNnQB and 1; refs around the tile and the chunk (2 tiles by default), not a multiple of 4, and 1
NN_CASES = [(1, 1), (1, 1030), (255, 511), (256, 512), (257, 513), (2047, 1023), (2048, 1025), (2049, 7), (300, 2501)]


@pytest.mark.parametrize("n,m", NN_CASES)
def test_sim_nn_matches_float64_brute_force_for_every_chunking(n, m):
    rng = np.random.default_rng(n * 7919 + m)
    q, r = _cloud(rng, n), _cloud(rng, m)
    assert nn_exempt_share(q, r) <= 0.01          # from the oracle alone: the index comparison below covers at least 99 %
    base = _nn3(q, r)
    check_nn(q, r, base["dist"], base["index"])
    for rchunk in (TILE, 2 * TILE, 3 * TILE):         # chunks of one object meet through the 64-bit atomic min: the same bits
        o = run3(lambda: simlib.sim_nn(q, r, rchunk=rchunk))
        assert o["plan"][3] == rchunk and o["plan"][4] == -(-n // QB) * -(-m // rchunk)
        for k in ("dist", "index", "keys"):
            assert o[k].tobytes() == base[k].tobytes(), (rchunk, k)


def test_sim_nn_duplicates_go_to_the_lowest_index():
    """Exact duplicates among the refs: no query is exempt, every index is compared exactly."""
    rng = np.random.default_rng(2)
    base = rng.uniform(0, 1, (700, 3)).astype(np.float32)
    r = np.concatenate([base, base, base[::-1]])                  # 2100 refs: every point three times, over several tiles and chunks
    for rchunk in (0, TILE, 2 * TILE):
        o = _nn3(base, r, rchunk=rchunk)
        assert (o["dist"] == 0).all()
        np.testing.assert_array_equal(o["index"], np.arange(700))
        np.testing.assert_array_equal(o["index"], eo.nn(base, r)[1])
    ring = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    for refs in (ring, ring[::-1].copy()):
        o = _nn3(np.zeros((1, 3), np.float32), np.concatenate([np.full((TILE + 3, 3), 9, np.float32), refs]), rchunk=TILE)
        assert float(o["dist"][0]) == 1.0 and int(o["index"][0]) == TILE + 3


def _check_sets(q, r, qs, rs, o):
    """Every non-empty set against the float64 brute force of that set (check_nn: distances within the bound, indices exactly
    wherever the oracle's runner-up gap exceeds float32 rounding), and the share of queries so exempted, over the whole call and from
    the oracle alone, at most 1 %."""
    qo, ro = np.concatenate([[0], np.cumsum(qs)]), np.concatenate([[0], np.cumsum(rs)])
    exempt = 0.0
    for s in np.flatnonzero(qs):
        qq, rr = q[qo[s]:qo[s + 1]], r[ro[s]:ro[s + 1]]
        exempt += nn_exempt_share(qq, rr) * len(qq)
        got = o["index"][qo[s]:qo[s + 1]] - ro[s]
        assert ((got >= 0) & (got < rs[s])).all(), f"set {s}: a neighbour outside the set"
        check_nn(qq, rr, o["dist"][qo[s]:qo[s + 1]], got)
    assert exempt / qs.sum() <= 0.01


def test_sim_nn_segmented_with_empty_sets():
    rng = np.random.default_rng(3)
    qs = np.array([0, 40, 0, 2100, 0, 1, 300, 0])
    rs = np.array([0, 7, 50, 1100, 0, 600, 1, 9])               # nothing at all; refs without queries; one ref; one query
    q, r = _cloud(rng, qs.sum(), 3.0), _cloud(rng, rs.sum(), 3.0)
    qo, ro = np.concatenate([[0], np.cumsum(qs)]), np.concatenate([[0], np.cumsum(rs)])
    o = _nn3(q, r, qo=qo, ro=ro, rchunk=TILE)
    np.testing.assert_array_equal(np.diff(o["prefix"]), [0, 1, 0, 2 * 3, 0, 2, 1, 0])
    _check_sets(q, r, qs, rs, o)
    # set by set: the same bits
    for s in np.flatnonzero(qs):
        one = _nn3(q[qo[s]:qo[s + 1]], r[ro[s]:ro[s + 1]], rchunk=2 * TILE)
        assert one["dist"].tobytes() == o["dist"][qo[s]:qo[s + 1]].tobytes()
        np.testing.assert_array_equal(one["index"] + ro[s], o["index"][qo[s]:qo[s + 1]])


def test_sim_nn_over_more_sets_than_one_plan_chunk():
    """1025 small sets, empties first and on both sides of the edge of nn_plan's first chunk of 1024 sets: the prefix of the work
    items is compared exactly, and nn_search finds every item's set in it (segment_of over shared offsets)."""
    rng = np.random.default_rng(31)
    n_sets = 1025
    qs, rs = rng.integers(1, 40, n_sets), rng.integers(1, 30, n_sets)
    empty = rng.random(n_sets) < 0.2
    empty[[0, 511, 1023]] = True
    empty[[1, 1022, 1024]] = False
    qs[empty] = 0
    rs[empty & (rng.random(n_sets) < 0.5)] = 0
    q, r = _cloud(rng, int(qs.sum()), 3.0), _cloud(rng, int(rs.sum()), 3.0)
    qo, ro = np.concatenate([[0], np.cumsum(qs)]), np.concatenate([[0], np.cumsum(rs)])
    o = _nn3(q, r, qo=qo, ro=ro)
    np.testing.assert_array_equal(o["prefix"], np.concatenate([[0], np.cumsum((qs > 0) & (rs > 0))]))
    assert qs[1024] > 0 and o["prefix"][1024] > 0
    _check_sets(q, r, qs, rs, o)


def test_sim_nn_writes_only_its_query_range():
    rng = np.random.default_rng(4)
    q, r = _cloud(rng, 5000), _cloud(rng, 3000)
    qo = np.array([100, 100, 2100, 4000], np.int64)             # queries [0, 100) and [4000, 5000) belong to no set
    ro = np.array([0, 7, 1500, 3000], np.int64)
    o = _nn3(q, r, qo=qo, ro=ro)
    for k, poison in (("dist", simlib.POISON_F32), ("index", simlib.POISON_I32), ("keys", np.uint64(0xA5A5A5A5A5A5A5A5))):
        rest = np.concatenate([o[k][:100], o[k][4000:]])
        assert rest.tobytes() == np.full(len(rest), poison, o[k].dtype).tobytes(), k
    for a, b, r0, r1 in ((100, 2100, 7, 1500), (2100, 4000, 1500, 3000)):
        assert nn_exempt_share(q[a:b], r[r0:r1]) <= 0.01
        check_nn(q[a:b], r[r0:r1], o["dist"][a:b], o["index"][a:b] - r0)
    # a narrower range of the same sets: only it is written, with the same bits
    part = _nn3(q, r, qo=qo, ro=ro, q_begin=1500, q_end=2600)
    assert part["dist"][1500:2600].tobytes() == o["dist"][1500:2600].tobytes()
    assert part["index"][1500:2600].tobytes() == o["index"][1500:2600].tobytes()
    for k, poison in (("dist", simlib.POISON_F32), ("index", simlib.POISON_I32)):
        rest = np.concatenate([part[k][:1500], part[k][2600:]])
        assert rest.tobytes() == np.full(len(rest), poison, part[k].dtype).tobytes(), k


# ---- surface sampling --------------------------------------------------------------------------------------------------------------

def _surface_sets(rng, nfs, nv=300):
    """One vertex array, the sets' faces one after the other; zero-area faces and vertex indices outside [0, V) sprinkled in (never
    on a set's first or last face).  -> (v, f, fo, v_oracle, f_oracle): the oracle mesh reads an outside index as an appended origin."""
    v = rng.uniform(-1, 1, (nv, 3)).astype(np.float32) + 2.0
    f = rng.integers(0, nv, (sum(nfs), 3)).astype(np.int32)
    fo = np.concatenate([[0], np.cumsum(nfs)]).astype(np.int64)
    for s, nf in enumerate(nfs):
        f[fo[s]], f[fo[s + 1] - 1] = (0, 1, 2), (3, 4, 5)                   # the first and the last face have area
        if nf < 8:
            continue
        mid = fo[s] + 1 + rng.choice(nf - 2, max(2, nf // 10), replace=False)
        half = len(mid) // 2
        f[mid[:half], 2] = f[mid[:half], 1]                                # zero area
        f[mid[half:], rng.integers(0, 3, len(mid) - half)] = rng.choice([-1, nv, nv + 5, -2 ** 31], len(mid) - half)
    f_or = np.where((f < 0) | (f >= nv), nv, f)
    return v, f, fo, np.concatenate([v, np.zeros((1, 3), np.float32)]), f_or


SURF_NF = [1, 1023, 1024, 1025, 2049, 37]           # around kCdfWG * kCdfPer = 1024 faces per round of surface_cdf


def test_sim_surface_cdf_and_test_mode_sampling():
    rng = np.random.default_rng(5)
    v, f, fo, v_or, f_or = _surface_sets(rng, SURF_NF)
    counts = [50, 700, 300, 513, 900, 64]
    oo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    u0s, rs, want_p, want_f = [], [], [], []
    for s, n in enumerate(counts):
        fs = f_or[fo[s]:fo[s + 1]]
        area = eo.face_areas(v_or, fs)
        cdf = np.cumsum(area)
        assert area[0] > 0 and area[-1] > 0
        face = rng.choice(np.flatnonzero(area > 1e-3 * area.max()), n)      # faces with an interval of their own on the CDF
        lo = np.where(face > 0, cdf[face - 1], 0.0)
        u0 = (lo + (0.25 + 0.5 * rng.uniform(size=n)) * (cdf[face] - lo)) / cdf[-1]         # away from the CDF's steps
        u0[0], face[0] = 0.0, 0                                             # searchsorted_left at 0: the first face
        u0[1], face[1] = 1.0 - 2.0 ** -53, len(fs) - 1                      # just below 1: the last face (it has area)
        r = rng.uniform(0, 1, (n, 2)).astype(np.float32)
        r[2], r[3] = (0.75, 0.75), (0.5, 0.5)                              # folded; exactly 1: not folded
        p, fc = eo.sample(v_or, fs, u0, r)
        np.testing.assert_array_equal(fc, face)
        u0s.append(u0), rs.append(r), want_p.append(p), want_f.append(fc + fo[s])
    assert (np.concatenate(rs).sum(1) > 1).mean() > 0.3
    u0, r, want, wface = np.concatenate(u0s), np.concatenate(rs), np.concatenate(want_p), np.concatenate(want_f)
    o = run3(lambda: simlib.sim_surface_sample(v, f, fo, oo, u0=u0, r=r))
    # the CDF: float64 face areas, per set, inclusive; the sums run in another order than numpy's
    for s in range(len(counts)):
        ref = np.cumsum(eo.face_areas(v_or, f_or[fo[s]:fo[s + 1]]))
        got = o["cdf"][fo[s]:fo[s + 1]]
        assert (np.abs(got - ref) <= 1e-6 * ref[-1]).all()
        # non-decreasing up to rounding: an entry is carry + (scan - own) + partial, at most 8 (tree) + 4 (lane) + 3 roundings of
        # sums no larger than the total, so two neighbours can be out of order by no more than that
        assert (np.diff(got) >= -16 * 2.0 ** -52 * ref[-1]).all()
    np.testing.assert_array_equal(o["face_index"], wface)
    L = np.abs(want).max()
    assert np.abs(o["points"] - want).max() <= 1e-6 * L
    # a sub-range of the output points: the rest untouched, the range bit-identical
    a, b = 777, 1600                                                     # inside set 2 ... inside set 4
    part = run3(lambda: simlib.sim_surface_sample(v, f, fo, oo, u0=u0, r=r, o_begin=a, o_end=b))
    assert part["points"][a:b].tobytes() == o["points"][a:b].tobytes() and part["face_index"][a:b].tobytes() == o["face_index"][a:b].tobytes()
    for k, poison in (("points", simlib.POISON_F32), ("face_index", simlib.POISON_I32)):
        rest = np.concatenate([part[k][:a], part[k][b:]])
        assert rest.tobytes() == np.full(rest.shape, poison, rest.dtype).tobytes(), k


def test_sim_surface_philox_mode_is_predicted_by_plain_python():
    """surface_sample drawing its own numbers against eval_oracle.sample fed with philox_ref.surface_randoms, whose Philox is held to
    the published known-answer vectors by tests/test_philox.py."""
    rng = np.random.default_rng(6)
    v, f, fo, v_or, f_or = _surface_sets(rng, [60, 1500], nv=40)
    counts = [300, 900]
    oo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    seed, stream, set_base = 0x1234_5678_9ABC_DEF0, 3, 4
    o = run3(lambda: simlib.sim_surface_sample(v, f, fo, oo, seed=seed, stream_id=stream, set_base=set_base))
    for s, n in enumerate(counts):
        u0, r = surface_randoms(n, set_base + s, stream, seed)
        for j in (0, 1, n - 1):                                          # the vectorised draw, spelled out in plain integers
            w = philox4x32_10((j, set_base + s, stream, 0), (seed & M32, seed >> 32))
            assert u0[j] == float((w[0] << 21) | (w[1] >> 11)) * 2.0 ** -53
            assert tuple(r[j]) == (np.float32(w[2] >> 8) * np.float32(2.0 ** -24), np.float32(w[3] >> 8) * np.float32(2.0 ** -24))
        assert 0 <= u0.min() and u0.max() < 1 and 0.3 < u0.mean() < 0.7 and 0.3 < r.mean() < 0.7
        p, fc = eo.sample(v_or, f_or[fo[s]:fo[s + 1]], u0, r)
        np.testing.assert_array_equal(o["face_index"][oo[s]:oo[s + 1]], fc + fo[s])
        assert np.abs(o["points"][oo[s]:oo[s + 1]] - p).max() <= 1e-6 * np.abs(p).max()
    other = run3(lambda: simlib.sim_surface_sample(v, f, fo, oo, seed=seed + 1, stream_id=stream, set_base=set_base))
    assert (other["points"] != o["points"]).any(1).mean() > 0.99


# ---- cropping to a box -------------------------------------------------------------------------------------------------------------

def _clip3(v, f, box, cap=None):
    return run3(lambda: simlib.sim_clip(v, f, box, cap))


def test_sim_clip_matches_the_float64_clipper():
    """Small triangles scattered over a cube, a rotated box through the middle of them: count, vertices, area, containment, and the
    triangles inside bit-unchanged in face order (geom_checks.check_clip_against_oracle, the GPU tier's comparison)."""
    rng = np.random.default_rng(7)
    centres = rng.uniform(2.5, 5.5, (1500, 1, 3))
    v = (centres + rng.normal(0, 0.12, (1500, 3, 3))).reshape(-1, 3).astype(np.float32)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)[rng.permutation(1500)]
    R, c, e = rotation_qr(rng), [4.1, 3.9, 4.2], [1.8, 1.2, 2.0]
    box = simlib.box15(c, R, e)
    o = _clip3(v, f, box)
    assert o["count"] == len(o["triangles"])
    counts = check_clip_against_oracle(v, f, o["triangles"], c, R, e, min_inside=20)
    assert {1, 2, 3} <= set(counts.tolist())                    # cut faces of several fan sizes
    per_blk = np.concatenate([counts, np.zeros((-len(counts)) % 256, np.int64)]).reshape(-1, 256).sum(1)
    np.testing.assert_array_equal(o["blk"], np.cumsum(per_blk) - per_blk)
    # a capacity below the total: the prefix, nothing past it
    for cap in (o["count"] // 2, 1, 0):
        part = _clip3(v, f, box, cap)
        assert part["count"] == o["count"] and part["triangles"].tobytes() == o["triangles"][:cap].tobytes()
    # everything outside, and no faces at all
    far = simlib.box15([40, 40, 40], np.eye(3), [1, 1, 1])
    assert _clip3(v, f, far)["count"] == 0
    assert _clip3(v, np.zeros((0, 3), np.int32), box)["count"] == 0


@pytest.mark.parametrize("nblk", [1, pytest.param(1023, marks=pytest.mark.slow), pytest.param(1024, marks=pytest.mark.slow),
                                  pytest.param(1025, marks=pytest.mark.slow), pytest.param(2049, marks=pytest.mark.slow)])
def test_sim_clip_of_whole_triangles_across_scan_chunks(nblk):
    """geom_checks.whole_triangle_case: a known number of triangles per face (one or none), clip_scan ending before, at and past its
    chunks of 1024 block totals.  The crop is v[f[inside]] bit for bit and the prefix of the block totals exact."""
    v, f, inside, R, centre, extent = whole_triangle_case(nblk)
    o = _clip3(v, f, simlib.box15(centre, R, extent))
    assert o["count"] == inside.sum()
    np.testing.assert_array_equal(o["triangles"], v[f[inside]])
    per_blk = np.concatenate([inside, np.zeros((-len(inside)) % 256, bool)]).reshape(-1, 256).sum(1)
    np.testing.assert_array_equal(o["blk"], np.cumsum(per_blk) - per_blk)


# ---- unprojection ------------------------------------------------------------------------------------------------------------------

PIXBLOCK = 1024            # kPixBlock: pixels per workgroup of unproject_count / _emit


def _unproject_case():
    """Ten views of bounds_oracle's scene at 37 x 29 (1073 pixels: no multiple of 1024 nor of 4, two blocks per frame) plus one frame with
    a degenerate pose, and seven objects over 1116 pairs = 2232 block totals: unproject_scan leaves its first and its second chunk."""
    sc = bo.Scene(width=37, height=29, fx=35.0, n_views=10, radius=3.0, seed=1)
    depth = np.stack([f["depth"] for f in sc.frames] + [sc.frames[0]["depth"]])
    inst = np.stack([f["inst"] for f in sc.frames] + [np.zeros((37, 29), np.int32)])
    inst[10, 10:29, 8:23], depth[10, 10:29, 8:23] = 9, 2.0            # id 9: a patch around the principal point, all four quadrants
    t_wc = np.stack([f["t_wc"] for f in sc.frames] + [sc.frames[0]["t_wc"].copy()])
    neg = np.flatnonzero((inst[1] == 3).ravel())[::5]
    depth[1].reshape(-1)[neg] = -1.5                                  # negative depth: ignored like depth 0
    assert (depth[inst > 0] == 0).sum() > 5 and len(neg) > 5
    t_wc[10, 2, :] = -0.0                                             # slot 10: z = -0 . xc + -0 . yc + -0 . d + -0: zeros of both signs
    cyc = lambda n, k0=0: [(int(s) % 10) for s in range(k0, k0 + n)]          # noqa: E731
    objs = [[(s, 3) for s in range(10)],
            [],                                                       # no pairs, in the middle
            [(s, 7) for s in cyc(300)] + [(-1, 7), (11, 7)] + [(s, 7) for s in cyc(300, 3)],      # two slots outside the store
            [(s, 3) for s in cyc(500, 7)],
            [(s, 11) for s in range(3)],                              # pairs, but no pixel carries the id
            [(10, 9)],
            []]                                                       # no pairs, at the end
    pairs = np.array([p for o in objs for p in o], np.int32).reshape(-1, 2)
    first = np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.int32)
    return sc, depth, inst, t_wc, objs, pairs, first


def _unproject_oracle(sc, depth, inst, t_wc, objs):
    pts, scale, per_blk = [], [], []
    nb = -(-depth[0].size // PIXBLOCK)
    for o in objs:
        op, os_ = [np.zeros((0, 3))], [np.zeros((0, 3))]
        for slot, oid in o:
            if not 0 <= slot < len(depth):
                per_blk.append(np.zeros(nb, np.int64))
                continue
            p, s = bo.unproject(depth[slot], inst[slot], t_wc[slot], sc.k4, oid)
            keep = ((inst[slot] == oid) & (depth[slot] > 0)).ravel()
            per_blk.append(np.concatenate([keep, np.zeros(nb * PIXBLOCK - keep.size, bool)]).reshape(nb, PIXBLOCK).sum(1))
            op.append(p), os_.append(s)
        pts.append(np.concatenate(op)), scale.append(np.concatenate(os_))
    return pts, scale, np.concatenate(per_blk)


@pytest.mark.slow
def test_sim_unproject_matches_the_checker_past_two_scan_chunks():
    sc, depth, inst, t_wc, objs, pairs, first = _unproject_case()
    ref, scale, per_blk = _unproject_oracle(sc, depth, inst, t_wc, objs)
    o = run3(lambda: simlib.sim_unproject(depth, inst, t_wc, sc.k4, pairs, first))
    assert o["nb"] == 2 and len(per_blk) == 2232
    np.testing.assert_array_equal(o["offsets"], np.concatenate([[0], np.cumsum([len(p) for p in ref])]))
    ex = np.cumsum(per_blk) - per_blk
    np.testing.assert_array_equal(o["blk"], ex)
    assert ex[1024] > 0 and ex[2048] > ex[1024]
    off = o["offsets"]
    assert off[1] == off[2] and off[4] == off[5] and off[6] == off[7] and off[1] > 300 and off[6] > off[5]
    for k, (p, s) in enumerate(zip(ref, scale)):
        got = o["points"][off[k]:off[k + 1]]
        # order (object, pair, pixel) and value: point by point, the GPU tier's bound
        assert (np.abs(got.astype(np.float64) - p) <= 6 * 2.0 ** -24 * s).all(), k
        lo, hi = o["bounds"][k, :3], o["bounds"][k, 3:]
        if len(p) == 0:
            assert (lo == np.inf).all() and (hi == -np.inf).all()
        else:
            np.testing.assert_array_equal(lo, got.min(0))              # exactly the extremes of what was emitted
            np.testing.assert_array_equal(hi, got.max(0))
    # object 5: z is a zero of either sign point by point; the bounds hold +0, by bits
    z = o["points"][off[5]:off[6], 2]
    assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
    assert o["bounds"][5, [2, 5]].view(np.uint32).tolist() == [0, 0]
    # a capacity below the total: the prefix, nothing past it
    for cap in (int(off[-1]) - 1, int(off[3]) + 5, 0):
        part = run3(lambda: simlib.sim_unproject(depth, inst, t_wc, sc.k4, pairs, first, cap))
        assert part["offsets"].tobytes() == off.tobytes() and part["points"].tobytes() == o["points"][:cap].tobytes()


def test_sim_unproject_small():
    """One scan chunk: the first two objects of the big case (an object without pairs last), and a call without pairs at all."""
    sc, depth, inst, t_wc, objs, _, _ = _unproject_case()
    objs = [objs[0], objs[5], []]
    pairs = np.array([p for o in objs for p in o], np.int32).reshape(-1, 2)
    first = np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.int32)
    ref, scale, per_blk = _unproject_oracle(sc, depth, inst, t_wc, objs)
    o = run3(lambda: simlib.sim_unproject(depth, inst, t_wc, sc.k4, pairs, first))
    np.testing.assert_array_equal(o["offsets"], np.concatenate([[0], np.cumsum([len(p) for p in ref])]))
    np.testing.assert_array_equal(o["blk"], np.cumsum(per_blk) - per_blk)
    for k in range(2):
        got = o["points"][o["offsets"][k]:o["offsets"][k + 1]]
        assert len(got) > 20 and (np.abs(got.astype(np.float64) - ref[k]) <= 6 * 2.0 ** -24 * scale[k]).all()
        np.testing.assert_array_equal(o["bounds"][k], np.concatenate([got.min(0), got.max(0)]))
    assert o["bounds"][1, [2, 5]].view(np.uint32).tolist() == [0, 0]
    none = run3(lambda: simlib.sim_unproject(depth, inst, t_wc, sc.k4, np.zeros((0, 2), np.int32), np.zeros(3, np.int32)))
    assert none["offsets"].tolist() == [0, 0, 0] and (none["bounds"][:, :3] == np.inf).all() and (none["bounds"][:, 3:] == -np.inf).all()


# ---- extents along candidate frames, moments, the order-preserving encoding --------------------------------------------------------

OBB_SIZES = [1, 511, 0, 512, 513, 1700]            # kObbTile = 512: below, at, past one tile; several tiles; one point; none


def _clouds(rng, sizes):
    parts = [(rng.standard_normal((n, 3)) * rng.uniform(0.05, 30.0) * (1.0, 2.0, 0.3) + rng.uniform(-3, 3, 3)).astype(np.float32) for n in sizes]
    return parts, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-object"])
@pytest.mark.parametrize("K", [1] + [pytest.param(k, marks=pytest.mark.slow) for k in (1023, 1024, 1025)])
def test_sim_obb_extents_match_the_checker_for_every_chunking(K, shared):
    """Against bounds_oracle.extents64 on the float32-centred points at the GPU tier's bound (2^-22 of the magnitude sum at the extreme
    point).  An object without points returns lo = +inf, hi = -inf (include/vmapstep.h), pinned here.  Minimum and maximum are exact,
    so every number of point chunks - one, two, seven, more than the object has tiles - gives the same bits."""
    rng = np.random.default_rng(K + shared)
    parts, off = _clouds(rng, OBB_SIZES)
    pts = np.concatenate(parts)
    rot = bo.random_rotations(rng, K if shared else K * len(OBB_SIZES)).astype(np.float32)
    rot = rot if shared else rot.reshape(len(OBB_SIZES), K, 3, 3)
    centre = np.stack([p.mean(0) if len(p) else np.zeros(3) for p in parts]).astype(np.float32)
    for c in (None, centre):
        lo, hi = run3(lambda: simlib.sim_obb_extents(pts, off, rot, c))
        assert (lo[2] == np.inf).all() and (hi[2] == -np.inf).all()
        for o in (0, 1, 3, 4, 5):
            lo64, hi64, slo, shi = bo.extents64(parts[o], rot if shared else rot[o], None if c is None else c[o])
            assert (np.abs(lo[o] - lo64) <= 2.0 ** -22 * slo).all() and (np.abs(hi[o] - hi64) <= 2.0 ** -22 * shi).all(), o
        assert (lo[0] == hi[0]).all()                                # one point
        for chunks in (1, 2, 7, 40):
            lo2, hi2 = run3(lambda: simlib.sim_obb_extents(pts, off, rot, c, chunks))
            assert lo2.tobytes() == lo.tobytes() and hi2.tobytes() == hi.tobytes(), chunks


def test_sim_obb_extents_enter_a_negative_zero_as_plus_zero():
    """Points in the plane z = 0 seen along the axes: every projection on the third row is a zero whose sign depends on the point;
    lo and hi hold +0 by bits, for every chunking (chunks with only -0 meet chunks with +0 through the integer atomics)."""
    rng = np.random.default_rng(9)
    p = rng.uniform(-1, 1, (1300, 3)).astype(np.float32)
    p[:, 2] = 0.0
    p[:600, :2] = -np.abs(p[:600, :2])                               # the first tile: every product with +row is -0 or +0 ...
    rot = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [0, 1, 0], [-0.0, -0.0, -1]]], np.float32)
    for chunks in (1, 3):
        lo, hi = run3(lambda: simlib.sim_obb_extents(p, np.array([0, 1300], np.int64), rot, None, chunks))
        assert lo[0, :, 2].view(np.uint32).tolist() == [0, 0] and hi[0, :, 2].view(np.uint32).tolist() == [0, 0]
        np.testing.assert_array_equal(lo[0, 0, :2], p[:, :2].min(0))
        np.testing.assert_array_equal(hi[0, 0, :2], p[:, :2].max(0))


def test_sim_enc_dec_round_trip_and_order():
    """enc_f32 / dec_f32: the round trip is the identity on bits, and unsigned order of the encoding is the order of the values
    (-0 just below +0).  A million random bit patterns and the edges of the format."""
    rng = np.random.default_rng(10)
    bits = rng.integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                        0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000], np.uint32)
    x = np.concatenate([special, bits]).view(np.float32)
    enc, dec = run3(lambda: simlib.sim_enc_dec(x))
    assert dec.view(np.uint32).tobytes() == x.view(np.uint32).tobytes()
    ok = ~np.isnan(x)
    e, v, b = enc[ok], x[ok], x[ok].view(np.uint32)
    order = np.argsort(e, kind="stable")
    e, v, b = e[order], v[order], b[order]
    assert (np.diff(v.astype(np.float64)) >= 0).all()                 # unsigned order of the code = order of the value
    same_code = np.diff(e.astype(np.int64)) == 0
    assert (b[1:][same_code] == b[:-1][same_code]).all()              # one code, one bit pattern
    assert enc[1] + 1 == enc[0] and enc[11] < enc[9] < enc[1] < enc[0] < enc[8] < enc[10]       # -inf < -max < -0 < +0 < max < inf


@pytest.mark.parametrize("centred", [False, True])
def test_sim_cloud_moments_match_float64_sums(centred):
    """Against numpy's float64 sums of the float64 terms (the float32 coordinates minus the float32 centre are exact in float64).
    Two things differ.  The ORDER of the additions: a lane adds ceil(n / 1024) terms one after the other and a tree of depth 10
    follows, numpy adds pairwise in about log2(n) + 8 levels; a sum of k roundings is within k 2^-53 of the sum of the terms'
    magnitudes.  And the PRODUCTS: numpy rounds x * y before it adds, the kernel's `s += x * y` may be contracted to a fused
    multiply-add whose product is not rounded (the device compiler and the executor's both contract), one more 2^-53 of every term.
    So |difference| <= (ceil(n / 1024) + 10 + log2(n) + 8 + 1) 2^-53 sum |term|."""
    rng = np.random.default_rng(11)
    sizes = [0, 1, 1023, 1024, 1025, 5000]
    parts, off = _clouds(rng, sizes)
    pts = np.concatenate(parts)
    centre = np.stack([p.mean(0) if len(p) else np.zeros(3) for p in parts]).astype(np.float32) if centred else None
    got = run3(lambda: simlib.sim_cloud_moments(pts, off, centre))
    assert not got[0].any()
    for o, n in enumerate(sizes):
        if n == 0:
            continue
        q = parts[o].astype(np.float64) - (centre[o].astype(np.float64) if centred else 0.0)
        x, y, z = q.T
        terms = np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z])
        k = -(-n // 1024) + 10 + np.log2(n) + 8 + 1
        assert (np.abs(got[o] - terms.sum(1)) <= k * 2.0 ** -53 * np.abs(terms).sum(1)).all(), o
    alone = run3(lambda: simlib.sim_cloud_moments(parts[5], np.array([0, 5000], np.int64), None if centre is None else centre[5:6]))
    assert alone[0].tobytes() == got[5].tobytes()                    # the order depends on the object alone
