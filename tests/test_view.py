"""CPU tier of the view renderer: the argument checks of vmapstep_view_* (no device is touched), the checker's composite against the
reference's own compositing functions, and the geometry header csrc/view_geometry.h - compiled into the host program
tests/tools/view_geometry_host.cpp - against the float64 checker and, bit for bit, against its float32 emulation."""
import ctypes

import numpy as np
import pytest

import view_oracle as vo
from vmap_amd import _lib

STD = vo.Standard


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return vo.build_host_program(tmp_path_factory.mktemp("view_host"))


def _dummy():
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256


def _cfg(width=96, height=64, samples=16, n_obj=4, pix=None):
    T = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    b, e = pix if pix is not None else (0, width * height)
    return _lib.ViewCfg(width, height, samples, n_obj, 90.0, 90.0, 47.5, 31.5, T, 0.05, b, e)


def _render(lib, cfg, p, hidden=32, n_pairs=0, ws_bytes=0):
    pp = _lib.Params()
    for t in range(_lib.NUM_FC):
        pp.fc[t] = _lib.Tensor(p, 0)
    pp.pe_B = _lib.Tensor(p, 0)
    sc = _lib.Tensor(p, 0)
    off = (ctypes.c_int64 * (cfg.n_obj + 1))(*([0] + [n_pairs] * cfg.n_obj))
    return lib.vmapstep_view_render(ctypes.byref(cfg), hidden, ctypes.byref(pp), ctypes.byref(sc), p, p, p, off, p, n_pairs, p, p, p, p, p, p, p,
                                    p, ws_bytes, None)


LIMITS = [("samples", dict(samples=64), dict(samples=65)), ("samples low", dict(samples=1), dict(samples=0)),
          ("n_obj", dict(n_obj=256), dict(n_obj=257)), ("n_obj low", dict(n_obj=1), dict(n_obj=0)),
          ("width", dict(width=16384, height=1), dict(width=16385, height=1)),
          ("height", dict(width=1, height=16384), dict(width=1, height=16385))]


@pytest.mark.parametrize("what,at,past", LIMITS, ids=[l[0] for l in LIMITS])
def test_view_entry_points_refuse_shapes_past_their_limits(what, at, past):
    """Each limit of the view section of include/vmapstep.h: the shape AT the limit passes the check and gets as far as the next one -
    the workspace, given here with zero bytes (VMAPSTEP_ERR_WORKSPACE); one past it is VMAPSTEP_ERR_UNSUPPORTED.  Both answers come
    before anything touches a device; no device pointer is read."""
    lib = _lib.load()
    buf, p = _dummy()
    nb = ctypes.c_size_t()
    for cfg, want, msg in ((_cfg(**at), -3, b"view workspace"), (_cfg(**past), -2, b"view limits")):
        assert lib.vmapstep_view_count(ctypes.byref(cfg), p, p, p, 0, None) == want and msg in lib.vmapstep_last_error(), what
        assert _render(lib, cfg, p) == want and msg in lib.vmapstep_last_error(), what
        assert lib.vmapstep_view_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nb)) == (0 if want == -3 else -2), what


def test_view_render_refuses_other_widths_and_too_many_samples():
    lib = _lib.load()
    buf, p = _dummy()
    cfg = _cfg(samples=64)
    assert _render(lib, cfg, p, hidden=64) == -2 and b"hidden 32 only" in lib.vmapstep_last_error()
    at = (2 ** 31 - 1) // 64                                  # n_pairs * samples = 2^31 - 64 < 2^31
    assert _render(lib, cfg, p, n_pairs=at) == -3 and b"view workspace" in lib.vmapstep_last_error()
    assert _render(lib, cfg, p, n_pairs=at + 1) == -2 and b"n_pairs * samples < 2^31" in lib.vmapstep_last_error()
    # a pixel range outside the image and inconsistent offsets are argument errors
    assert lib.vmapstep_view_count(ctypes.byref(_cfg(pix=(0, 96 * 64 + 1))), p, p, p, 0, None) == -1
    assert lib.vmapstep_view_count(ctypes.byref(_cfg(pix=(10, 5))), p, p, p, 0, None) == -1
    assert lib.vmapstep_view_count(ctypes.byref(_cfg()), None, p, p, 0, None) == -1


def test_view_workspace_holds_images_block_totals_and_plan():
    """vl::view_layout: n_obj images of 80 KiB, one int64 per (object, 64-pixel block) of the range, 768 plan entries of 16 bytes."""
    lib = _lib.load()
    nb = ctypes.c_size_t()
    up = lambda x: (x + 255) // 256 * 256
    for n_obj, pix in ((4, (0, 96 * 64)), (21, (37, 5000)), (1, (5, 5))):
        assert lib.vmapstep_view_workspace_bytes(ctypes.byref(_cfg(n_obj=n_obj, pix=pix)), ctypes.byref(nb)) == 0
        blocks = -(-(pix[1] - pix[0]) // 64)
        assert nb.value == up(n_obj * 81920) + up(n_obj * blocks * 8) + up(768 * 16)
    assert ctypes.sizeof(_lib.ViewCfg) == 120 and _lib.ViewCfg.pix_begin.offset == 104


def test_checker_composite_equals_the_reference_functions():
    """The checker's single-object composite (float64) against the reference's occupancy_to_termination + render (float32 torch) on
    random occupancies, S = 64.  Tolerance: the float32 evaluation rounds free_j = 1 - occ_j + 1e-10 twice (2u each, u = 2^-24), the
    cumulative product of up to 63 of them 63 times, the product with occ_i and with the value once each, and the sum of 64 terms at
    most 63 times per term: (2 * 63 + 63 + 2 + 63) u = 254 u relative to sum_i |w_i v_i| <= max |v| (the weights sum to <= 1).  So
    |difference| <= 254 * 2^-24 * max |v| = 1.52e-5 max |v|."""
    import torch
    from oracle import ref_runner
    if not ref_runner.reference_available():
        pytest.skip("the reference's modules are not available (oracle/_ref is built by build())")
    rr = ref_runner._import_reference()["render_rays"]
    rng = np.random.default_rng(3)
    P, S = 257, 64
    occ = rng.random((P, S)).astype(np.float32)
    occ[:40] *= np.float32(0.05)                       # thin media: many terms carry weight
    occ[40:60, 5] = 1.0                                # an opaque sample: free = 1e-10
    t = np.sort(rng.random((P, S)).astype(np.float32) * 5, 1)
    rgb = rng.random((P, S, 3)).astype(np.float32)
    term = rr.occupancy_to_termination(torch.from_numpy(occ))
    ref_d = rr.render(term, torch.from_numpy(t)).numpy()
    ref_c = rr.render(term[..., None], torch.from_numpy(rgb), dim=-2).numpy()
    ref_o = term.sum(-1).numpy()
    got = vo.composite(P, np.ones((1, P), bool), t[None], occ[None], rgb[None])
    tol = 254 * 2.0 ** -24
    for name, a, b, vmax in (("depth", got["depth"], ref_d, 5.0), ("colour", got["color"], ref_c, 1.0), ("opacity", got["opacity"], ref_o, 1.0)):
        err = np.abs(a - b).max()
        print(f"{name}: max |checker - reference| {err:.3e} (tolerance {tol * vmax:.3e})")
        assert err <= tol * vmax, name
    assert (got["instance"] == 0).all()


@pytest.mark.parametrize("view", range(len(STD.VIEWS)))
def test_host_geometry_against_the_checker(host_exe, tmp_path, view):
    """csrc/view_geometry.h as g++ compiles it (-O2 -ffp-contract=off) on the standard scene: bit-identical to the checker's float32
    emulation (hits everywhere; t_near and dt wherever hit), and against the float64 checker outside the edge pixels (any object's
    float64 |t_far - t_near| < 1e-4; their share must stay <= 1 %): equal hit sets, t_near and dt within view_oracle.geometry_bound
    (derived there from the operation order; the division amplifies: eps_t ~ (eps_ob + t eps_db) / |db|)."""
    T = vo.ring_pose(*STD.VIEWS[view])
    args = (T, STD.k4(), STD.W, STD.H, STD.boxes(), STD.S, STD.MIN_DEPTH)
    hit, tn, dt = vo.run_host_program(host_exe, tmp_path, *args)
    e_hit, e_tn, e_dt = vo.geometry32(*args)
    assert np.array_equal(hit, e_hit)
    assert np.array_equal(tn[hit].view(np.uint32), e_tn[hit].view(np.uint32)) and np.array_equal(dt[hit].view(np.uint32), e_dt[hit].view(np.uint32))
    hit64, tn64, tf64, dt64, _ = vo.geometry64(*args)
    edge = vo.edge_pixels(tn64, tf64)
    print(f"view {view}: hits per pixel max {hit64.sum(0).max()}, mean {hit64.sum(0).mean():.2f}; edge pixels {edge.sum()} of {edge.size}")
    assert edge.mean() <= 0.01
    ok = ~edge
    assert np.array_equal(hit[:, ok], hit64[:, ok])
    b_tn, b_dt = vo.geometry_bound(*args)
    m = hit64 & ok[None]
    e1, e2 = np.abs(tn.astype(np.float64) - tn64)[m], np.abs(dt.astype(np.float64) - dt64)[m]
    print(f"   max |t_near - float64| {e1.max():.3e} (bound there {b_tn[m][e1.argmax()]:.3e}), max |dt - float64| {e2.max():.3e} "
          f"(bound there {b_dt[m][e2.argmax()]:.3e}); largest bound {b_tn[m].max():.3e}")
    assert (e1 <= b_tn[m]).all() and (e2 <= b_dt[m]).all()


def test_host_geometry_special_rays(host_exe, tmp_path):
    """An axis-aligned pose with an integer principal point (a pixel column and row with an exactly zero direction component: slabs
    parallel to the ray divide by zero), a camera inside a box (t_near clamped to min_depth) and a box behind the camera (never
    hit): the host program equals the emulation bit for bit, and the two special boxes behave as the contract says."""
    W, H = 32, 24
    k4 = (40.0, 40.0, 16.0, 12.0)
    T = np.eye(4, dtype=np.float32)
    boxes = [vo.Box((0, 0, 2), np.eye(3), (1, 1, 1)), vo.Box((0, 0, 0), np.eye(3), (1, 1, 1)), vo.Box((0, 0, -3), np.eye(3), (1, 1, 1)),
             vo.Box((0.5, 0, 2), np.eye(3), (1, 2, 0.5))]                   # x face at 0: the column w = cx lies ON a slab plane
    args = (T, k4, W, H, boxes, 5, 0.05)
    hit, tn, dt = vo.run_host_program(host_exe, tmp_path, *args)
    e_hit, e_tn, e_dt = vo.geometry32(*args)
    assert np.array_equal(hit, e_hit)
    assert np.array_equal(tn[hit].view(np.uint32), e_tn[hit].view(np.uint32)) and np.array_equal(dt[hit].view(np.uint32), e_dt[hit].view(np.uint32))
    assert hit[1].all() and (tn[1] == np.float32(0.05)).all()                 # inside: every ray leaves the box, from min_depth on
    assert not hit[2].any()                                                   # behind the camera
    centre = 16 * H + 12
    assert hit[0, centre] and tn[0, centre] == np.float32(1.5) and dt[0, centre] == np.float32(0.2)
    # on the face: ta = 0 / 0 is dropped, tb = 1 / 0 = +inf stays on both sides: t_near = +inf, a miss - and its neighbour column hits
    assert not hit[3, centre] and hit[3, centre + H] and tn[3, centre + H] == np.float32(1.75)
