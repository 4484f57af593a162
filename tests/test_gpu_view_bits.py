"""The view renderer against its recorded bits (tests/golden/view_bits.npz, written by tests/golden/make_view_goldens.py at the last
commit that had separate single-group kernels): every image, pair record, offset, count and sample buffer of every case is equal bit
for bit - floats compared as uint32, so -0.0 and NaN payloads count; the buffers too large for the fixture by their SHA-256.  No
tolerance: nothing the blocks combine is a float sum, so a differing bit is a change of the arithmetic, to be explained from the code."""
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("std32", "std32_range", "cap32", "mixed", "mixed_cap")


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLDEN, "view_bits.npz")) as z:
        return {k: z[k] for k in z.files}


def recorder():
    """The recording script as a module: its cases() and record() are the one definition of what the fixture holds."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_view_goldens
    finally:
        sys.path.remove(GOLDEN)
    return make_view_goldens


@pytest.fixture(scope="module")
def rendered():
    """Every case rendered once."""
    return recorder().cases()


def test_the_fixture_holds_every_case(recorded):
    assert {k.split("/")[0] for k in recorded} == set(CASES)
    for case, names in (("std32", ("depth", "color", "opacity", "instance", "overflow", "n_pairs", "pairs", "offsets", "sample_occ", "sample_rgb")),
                        ("std32_range", ("depth", "color", "opacity", "instance", "n_pairs", "bands")),
                        ("cap32", ("depth", "color", "opacity", "instance", "overflow")),
                        ("mixed", ("depth", "color", "opacity", "instance", "pairs", "offsets", "sample_occ", "sample_rgb")),
                        ("mixed_cap", ("depth", "color", "opacity", "instance", "overflow"))):
        assert {k.split("/")[1] for k in recorded if k.startswith(case + "/")} == set(names), case
    assert recorded["std32_range/bands"] >= 3 and recorded["cap32/overflow"] > 0 and recorded["mixed_cap/overflow"] > 0


@pytest.mark.parametrize("case", CASES)
def test_view_bits_equal_the_recorded_bits(recorded, rendered, case):
    keys = sorted(k for k in recorded if k.startswith(case + "/"))
    assert keys == sorted(k for k in rendered if k.startswith(case + "/"))
    for k in keys:
        want, got = recorded[k], rendered[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        if not np.array_equal(got, want):
            differ = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
            pytest.fail(f"{k}: {differ.size} of {want.size} words differ, first at {differ[:8].tolist()}")


def test_the_single_group_entry_points_give_the_recorded_bits(recorded):
    """vmapstep_view_workspace_bytes / _count / _render called directly on the ``std32`` scene (render_view goes through the scene entry
    points, so nothing else runs these three on a device): their own 768-entry workspace, every output equal to the fixture."""
    import ctypes
    import torch
    import view_oracle as vo
    from test_gpu_scene_view import CENTERS32
    from test_gpu_view import B3, stacked
    from vmap_amd import _devmem, _lib, render, synth
    mk, STD, dev = recorder(), vo.Standard, "cuda:0"
    n, S, P = 4, STD.S, STD.W * STD.H
    fc, pe_B, scale = stacked(synth.make_params(n, 32, seed=5))
    lib = _lib.load()
    pp = _lib.Params()
    for t, p in enumerate(fc):
        pp.fc[t] = _lib.Tensor(p.data_ptr(), p.stride(0))
    pp.pe_B = _lib.Tensor(pe_B.data_ptr(), pe_B.stride(0))
    sc = _lib.Tensor(scale.data_ptr(), 1)
    T = vo.ring_pose(*STD.VIEWS[0])
    cfg = _lib.ViewCfg(STD.W, STD.H, S, n, *STD.k4(), (ctypes.c_float * 16)(*T.reshape(-1)), STD.MIN_DEPTH, 0, P)
    ws, ws_ptr, nbytes = _devmem.workspace(lib, lib.vmapstep_view_workspace_bytes, dev, ctypes.byref(cfg))
    up = lambda x: (x + 255) // 256 * 256
    assert nbytes == up(n * 81920) + up(n * (P // 64) * 8) + up(768 * 16)
    boxes_d = torch.from_numpy(render._box_rows([B3(b) for b in STD.boxes()], n)).to(dev)
    centers_d = torch.from_numpy(CENTERS32).to(dev)
    off_d = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _lib.check(lib.vmapstep_view_count(ctypes.byref(cfg), boxes_d.data_ptr(), off_d.data_ptr(), ws_ptr, nbytes, _devmem.stream(dev)), lib)
    off_h = off_d.cpu().numpy().copy()
    m = int(off_h[-1])
    out = dict(pairs=torch.empty(m, 4, dtype=torch.int32, device=dev), sample_occ=torch.empty(m, S, device=dev),
               sample_rgb=torch.empty(m, S, 3, device=dev), depth=torch.zeros(STD.W, STD.H, device=dev), color=torch.zeros(STD.W, STD.H, 3, device=dev),
               opacity=torch.zeros(STD.W, STD.H, device=dev), instance=torch.full((STD.W, STD.H), -1, dtype=torch.int32, device=dev))
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.vmapstep_view_render(ctypes.byref(cfg), 32, ctypes.byref(pp), ctypes.byref(sc), boxes_d.data_ptr(), centers_d.data_ptr(),
                                        off_d.data_ptr(), off_h.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), out["pairs"].data_ptr(), m,
                                        out["sample_occ"].data_ptr(), out["sample_rgb"].data_ptr(), out["depth"].data_ptr(), out["color"].data_ptr(),
                                        out["opacity"].data_ptr(), out["instance"].data_ptr(), overflow.data_ptr(), ws_ptr, nbytes,
                                        _devmem.stream(dev)), lib)
    torch.cuda.synchronize()
    got = {}
    mk.record(got, "std32", overflow=np.int64(int(overflow.item())), n_pairs=np.int64(m), offsets=off_h, **out)
    assert sorted(got) == sorted(k for k in recorded if k.startswith("std32/"))
    for k, x in got.items():
        assert x.dtype == recorded[k].dtype and np.array_equal(x, recorded[k]), k


def test_a_digest_is_the_sha256_of_the_bits():
    """What a /sha256 key holds, pinned on a known array: the digest of the uint32 view's bytes."""
    mk = recorder()
    x = np.arange(mk.FULL_BYTES // 4 + 1, dtype=np.float32)
    out = {}
    mk.record(out, "c", big=x, small=x[:3])
    assert out["c/big/sha256"].tobytes() == hashlib.sha256(x.view(np.uint32).tobytes()).digest() and tuple(out["c/big/shape"]) == x.shape
    assert out["c/small"].dtype == np.uint32 and np.array_equal(out["c/small"], x[:3].view(np.uint32))
