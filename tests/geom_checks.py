"""Comparison helpers the GPU tier (tests/test_gpu_mesh.py, tests/test_gpu_eval.py) and the CPU executor tier
(tests/test_kernel_sim_geom.py) share: one definition of what "equals the float64 checker" means for a mesh and for nearest neighbours."""
import numpy as np

import eval_oracle as eo
import mesh_oracle as mo


def nn_bound(q, r):
    """(d64, i64, bound): the float64 brute force and the float32 bound 1e-6 (d + L) every nearest-neighbour comparison uses."""
    q64, r64 = np.asarray(q, np.float64), np.asarray(r, np.float64)
    d64, i64 = eo.nn(q64, r64)
    L = max(np.abs(q64).max(), np.abs(r64).max())
    return d64, i64, 1e-6 * (d64 + L)


def nn_exempt_share(q, r):
    """The share of queries whose index check_nn does not compare: the float64 runner-up gap is within float32 rounding (2 x bound).
    Computed from the oracle alone."""
    _, _, bound = nn_bound(q, r)
    return float((eo.runner_up_gap(np.asarray(q, np.float64), np.asarray(r, np.float64)) <= 2 * bound).mean())


def check_nn(q, r, d, i, check_index=True):
    q64, r64 = np.asarray(q, np.float64), np.asarray(r, np.float64)
    d64, i64, bound = nn_bound(q, r)
    err = np.abs(d.astype(np.float64) - d64)
    assert (err <= bound).all(), f"worst {err.max():.3g} vs bound {bound[err.argmax()]:.3g}"
    if check_index:
        sep = eo.runner_up_gap(q64, r64) > 2 * bound
        np.testing.assert_array_equal(i[sep], i64[sep])
        # the chosen ref is (within the bound) a nearest one wherever it differs
        dd = np.linalg.norm(q64 - r64[i], axis=1)
        assert (np.abs(dd - d64) <= 2 * bound).all()


def check_mesh_against_oracle(vol, gv, gf, gn, affine=None, level=0.5):
    """Faces exactly; vertices within 1e-5 (of the coordinates' size under an affine); normals within 1e-4 wherever the interpolated
    gradient is not (nearly) zero.  gn None: no normals to compare."""
    v, f, n, _ = mo.marching_cubes(vol, level, affine)
    np.testing.assert_array_equal(gf, f)
    assert gv.shape == v.shape and np.abs(gv - v).max() < 1e-5 * (1 if affine is None else np.abs(v).max() + 1)
    if gn is None:
        return
    g = mo.gradient(vol)
    _, _, _, eid = mo.marching_cubes(vol, level)
    pt, ax = eid // 3, eid % 3
    idx = np.stack(np.unravel_index(pt, vol.shape), -1)
    idx1 = idx.copy()
    idx1[np.arange(len(idx)), ax] += 1
    ok = (np.linalg.norm(g[tuple(idx.T)], axis=1) > 1e-6) | (np.linalg.norm(g[tuple(idx1.T)], axis=1) > 1e-6)
    ok &= np.linalg.norm(n, axis=1) > 0.5
    assert np.abs(gn[ok] - n[ok]).max() < 1e-4


def rotation_qr(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def whole_triangle_case(nblk):
    """``nblk`` blocks of 256 faces (the last one partial): every triangle lies wholly inside the box or wholly beyond one of its planes,
    so the crop is v[f[inside]] bit for bit, in face order.  Runs of whole blocks keep nothing: totals of zero inside the scan.
    -> (v, f, inside, R, centre, extent)"""
    rng = np.random.default_rng(nblk)
    nf = 256 * nblk - 5
    R = rotation_qr(rng)
    centre, extent = np.array([4.1, 3.9, 4.2]), np.array([1.8, 1.2, 2.0])
    inside = rng.random(nf) < 0.5
    if nblk > 8:
        inside[256 * 3:256 * 7] = False
        inside[256 * (nblk - 4):256 * (nblk - 2)] = False
    inside[[0, nf - 1]] = True
    # local centres: inside at least 0.1 from every plane, outside at least 0.1 beyond the +- plane of one axis; triangles of 0.02
    loc = rng.uniform(-1, 1, (nf, 3)) * (extent / 2 - 0.1)
    ax = rng.integers(0, 3, nf)
    out = ~inside
    loc[out, ax[out]] = (rng.choice([-1.0, 1.0], out.sum()) * (extent[ax[out]] / 2 + 0.1 + rng.uniform(0, 1, out.sum())))
    v = ((loc @ R.T + centre)[:, None, :] + rng.uniform(-0.02, 0.02, (nf, 3, 3))).reshape(-1, 3).astype(np.float32)
    f = np.arange(3 * nf, dtype=np.int32).reshape(-1, 3)
    f = f[:, rng.permutation(3)]
    return v, f, inside, R, centre, extent


def check_clip_against_oracle(v, f, tri32, center, R, extent, min_inside=100):
    """A cropped soup against eo.clip_mesh on the float32 box: the count exactly, vertices (the bulk within 1e-5 L, all within 1e-3 L: a
    cut along an edge nearly parallel to its plane is ill-conditioned in float32), the area within 1e-5, containment, and the triangles
    wholly inside the box bit-unchanged at their place in face order."""
    box32 = [np.float32(center).astype(np.float64), np.asarray(R).astype(np.float32).astype(np.float64),
             np.asarray(extent).astype(np.float32).astype(np.float64)]
    want = eo.clip_mesh(v, f, *box32)
    tri = tri32.astype(np.float64)
    assert len(tri) == len(want)
    L = np.abs(want).max()
    err = np.abs(tri - want).max(axis=(1, 2))
    assert np.quantile(err, 0.999) <= 1e-5 * L and err.max() <= 1e-3 * L
    assert abs(eo.soup_area(tri) - eo.soup_area(want)) <= 1e-5 * eo.soup_area(want)
    local = (tri.reshape(-1, 3) - box32[0]) @ box32[1]
    assert (np.abs(local) <= box32[2] / 2 + 1e-5 * L).all()
    loc_v = (v.astype(np.float64) - box32[0]) @ box32[1]
    inside = (np.abs(loc_v[f]) < box32[2] / 2 - 1e-3).all(axis=(1, 2))
    assert inside.sum() > min_inside
    counts = np.array([max(len(eo.clip_polygon(v[x].astype(np.float64), *box32)) - 2, 0) for x in f])
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    np.testing.assert_array_equal(tri32[first[inside]], v[f[inside]])
    return counts
