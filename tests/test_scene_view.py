"""CPU tier of the scene view (field groups: the scene paragraph of the view section of include/vmapstep.h): the argument checks of
vmapstep_scene_view_* (no device is touched), the workspace formula, the group struct against the C compiler's layout, the facts about
the standard mixed scene the GPU tier relies on, and the mixed-sample-count checker against view_oracle.composite."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import scene_view_oracle as so
import view_oracle as vo
from vmap_amd import _lib

STD = vo.Standard
ROOT = vo.ROOT


def _dummy():
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256


def _cfg(width=96, height=64, pix=None):
    T = (ctypes.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    b, e = pix if pix is not None else (0, width * height)
    return _lib.ViewCfg(width, height, 0, 0, 90.0, 90.0, 47.5, 31.5, T, 0.05, b, e)           # samples, n_obj: not read


class Scene:
    """A group array with dummy (never dereferenced) parameter pointers."""
    def __init__(self, p, specs):
        self.pp = _lib.Params()
        for t in range(_lib.NUM_FC):
            self.pp.fc[t] = _lib.Tensor(p, 0)
        self.pp.pe_B = _lib.Tensor(p, 0)
        self.sc = _lib.Tensor(p, 0)
        self.n = len(specs)
        self.n_obj = sum(s[1] for s in specs)
        self.arr = (_lib.ViewGroup * max(self.n, 1))(*[_lib.ViewGroup(h, n, s, 0, ctypes.pointer(self.pp), ctypes.pointer(self.sc)) for h, n, s in specs])


def _calls(lib, cfg, sc, p, pairs_per_obj=0, ws_bytes=0):
    """(workspace_bytes, count, render) statuses with their messages."""
    nb = ctypes.c_size_t()
    out = []
    out.append((lib.vmapstep_scene_view_workspace_bytes(ctypes.byref(cfg), sc.arr, sc.n, ctypes.byref(nb)), lib.vmapstep_last_error()))
    out.append((lib.vmapstep_scene_view_count(ctypes.byref(cfg), sc.arr, sc.n, p, p, p, ws_bytes, None), lib.vmapstep_last_error()))
    off = (ctypes.c_int64 * (max(sc.n_obj, 0) + 1))(*[pairs_per_obj * k for k in range(max(sc.n_obj, 0) + 1)])
    out.append((lib.vmapstep_scene_view_render(ctypes.byref(cfg), sc.arr, sc.n, p, p, p, off, p, pairs_per_obj * max(sc.n_obj, 0), p, p, p, p, p, p, p,
                                               p, ws_bytes, None), lib.vmapstep_last_error()))
    return out


LIMITS = [("groups", [(32, 1, 16)] * 4, [(32, 1, 16)] * 5), ("groups low", [(32, 1, 16)], []),
          ("hidden", [(256, 1, 16)], [(288, 1, 16)]), ("hidden step", [(64, 1, 16)], [(48, 1, 16)]),
          ("samples", [(32, 2, 64), (128, 1, 64)], [(32, 2, 16), (128, 1, 65)]), ("samples low", [(32, 2, 1), (128, 1, 1)], [(32, 2, 0), (128, 1, 1)]),
          ("objects", [(32, 255, 16), (128, 1, 48)], [(32, 255, 16), (128, 2, 48)])]


@pytest.mark.parametrize("what,at,past", LIMITS, ids=[l[0] for l in LIMITS])
def test_scene_entry_points_refuse_shapes_past_their_limits(what, at, past):
    """Each new limit: the shape AT the limit passes the checks and gets as far as the workspace, given here with zero bytes
    (VMAPSTEP_ERR_WORKSPACE); one past it is VMAPSTEP_ERR_UNSUPPORTED.  Both before anything touches a device: no device pointer is
    read, no parameter pointer followed."""
    lib = _lib.load()
    buf, p = _dummy()
    ok = _calls(lib, _cfg(), Scene(p, at), p)
    assert ok[0][0] == 0, what
    assert ok[1][0] == -3 and b"scene view workspace" in ok[1][1], what
    assert ok[2][0] == -3 and b"scene view workspace" in ok[2][1], what
    for rc, msg in _calls(lib, _cfg(), Scene(p, past), p):
        assert rc == -2 and b"scene view limits" in msg, (what, rc, msg)


def test_scene_render_refuses_2_to_31_samples_and_bad_arguments():
    lib = _lib.load()
    buf, p = _dummy()
    # two groups, one object each: pairs * 64 + pairs * 64 = 2^31 - 128 at the limit, 2^31 one past it
    at = (2 ** 31) // 128 - 1
    sc = Scene(p, [(32, 1, 64), (128, 1, 64)])
    rc, msg = _calls(lib, _cfg(), sc, p, pairs_per_obj=at)[2]
    assert rc == -3 and b"scene view workspace" in msg
    rc, msg = _calls(lib, _cfg(), sc, p, pairs_per_obj=at + 1)[2]
    assert rc == -2 and b"samples of all groups < 2^31" in msg
    # the sample counts are the groups' own: the same pairs with 64 and 1 samples are far below the limit
    rc, msg = _calls(lib, _cfg(), Scene(p, [(32, 1, 64), (128, 1, 1)]), p, pairs_per_obj=at + 1)[2]
    assert rc == -3
    one = Scene(p, [(64, 1, 16)])
    nb = ctypes.c_size_t()
    assert lib.vmapstep_scene_view_count(ctypes.byref(_cfg(pix=(0, 96 * 64 + 1))), one.arr, 1, p, p, p, 0, None) == -1
    assert lib.vmapstep_scene_view_count(ctypes.byref(_cfg(pix=(10, 5))), one.arr, 1, p, p, p, 0, None) == -1
    assert lib.vmapstep_scene_view_count(ctypes.byref(_cfg()), one.arr, 1, None, p, p, 0, None) == -1
    assert lib.vmapstep_scene_view_workspace_bytes(ctypes.byref(_cfg()), None, 1, ctypes.byref(nb)) == -1
    # offsets that do not end at n_pairs
    off = (ctypes.c_int64 * 2)(0, 5)
    assert lib.vmapstep_scene_view_render(ctypes.byref(_cfg()), one.arr, 1, p, p, p, off, p, 6, p, p, p, p, p, p, p, p, 0, None) == -1


def image_bytes(hidden):
    return 81920 if hidden == 32 else 4 * (-(-(4 * hidden * hidden + 253 * hidden + 72) // 1024) * 1024)


def test_scene_workspace_holds_group_images_block_totals_and_plan():
    """vl::scene_layout as include/vmapstep.h documents it: group after group n_obj_g images (80 KiB split images at hidden 32, the
    float32 image of the point query otherwise), one int64 per (object, 64-pixel block), 4 * 2048 + 256 plan entries of 16 bytes.
    The wide image is what vmapstep_query_workspace_bytes asks for one object."""
    lib = _lib.load()
    buf, p = _dummy()
    nb, q = ctypes.c_size_t(), ctypes.c_size_t()
    up = lambda x: (x + 255) // 256 * 256
    for specs, pix in (([(32, 4, 16), (128, 1, 48)], (0, 96 * 64)), ([(256, 1, 64)], (37, 5001)), ([(64, 3, 5), (32, 20, 16), (160, 2, 7), (96, 1, 1)], (5, 5))):
        sc = Scene(p, specs)
        assert lib.vmapstep_scene_view_workspace_bytes(ctypes.byref(_cfg(pix=pix)), sc.arr, sc.n, ctypes.byref(nb)) == 0
        blocks = -(-(pix[1] - pix[0]) // 64)
        assert nb.value == sum(up(n * image_bytes(h)) for h, n, _ in specs) + up(sc.n_obj * blocks * 8) + up((4 * 2048 + 256) * 16)
    for h in range(64, 257, 32):
        assert lib.vmapstep_query_workspace_bytes(h, ctypes.byref(q)) == 0 and q.value == up(image_bytes(h))


def test_group_struct_matches_the_c_layout(tmp_path):
    """sizeof / offsets of vmapstep_view_group as gcc lays out include/vmapstep.h against the ctypes structure."""
    src = tmp_path / "group_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmapstep.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", '
                   'sizeof(vmapstep_view_group), offsetof(vmapstep_view_group, samples), offsetof(vmapstep_view_group, params), '
                   'offsetof(vmapstep_view_group, pe_scale), VMAPSTEP_VIEW_MAX_GROUPS); return 0; }\n')
    exe = tmp_path / "group_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    G = _lib.ViewGroup
    assert got == [ctypes.sizeof(G), G.samples.offset, G.params.offset, G.pe_scale.offset, _lib.VIEW_MAX_GROUPS] and got[0] == 32


@pytest.mark.parametrize("view", range(len(STD.VIEWS)))
def test_the_standard_mixed_scene_is_what_the_gpu_tier_assumes(view):
    """The room box contains the camera: every pixel hits it from min_depth on, t_far within (5.0, 9.1); at most 5 boxes per pixel;
    edge pixels <= 1 %."""
    T = vo.ring_pose(*STD.VIEWS[view])
    groups = [so.Group(STD.boxes(), 16), so.Group([so.ROOM], 48)]
    hit, tn, tf, dt, _ = so.geometry64(T, STD.k4(), STD.W, STD.H, groups, STD.MIN_DEPTH)
    assert hit[4].all() and (tn[4] == np.float64(np.float32(STD.MIN_DEPTH))).all()
    # measured here: t_far 5.896 .. 8.192, 5.644 .. 9.041 and from 5.099 in the third view: the room is 5 - 9 m along a ray
    assert 5.0 < tf[4].min() and tf[4].max() < 9.1
    assert hit.sum(0).max() <= 5
    edge = vo.edge_pixels(tn, tf)
    print(f"view {view}: room t_far {tf[4].min():.3f} .. {tf[4].max():.3f}; hits per pixel max {hit.sum(0).max()}; edge pixels {edge.mean():.4%}")
    assert edge.mean() <= 0.01
    h32, tn32, dt32 = so.geometry32(T, STD.k4(), STD.W, STD.H, groups, STD.MIN_DEPTH)
    assert np.array_equal(h32[:, ~edge], hit[:, ~edge])
    # a group's rows are view_oracle's with the group's S: dt of the room is (t_far - t_near) / 48
    assert np.allclose(dt32[4], (tf[4] - tn[4]) / 48, rtol=1e-5)


def test_mixed_checker_equals_the_composite_when_all_groups_share_one_sample_count():
    """scene_view_oracle.composite (per-object sample counts, padded) against view_oracle.composite on random samples with one S for
    all objects: the same arrays, bit for bit; and with a shorter object the result equals view_oracle.composite on that object's
    samples extended by empty ones (occupancy 0 at a depth behind everything)."""
    rng = np.random.default_rng(11)
    n, P, S = 5, 300, 6
    hit = rng.random((n, P)) < 0.6
    t = np.sort(rng.random((n, P, S)) * 4, 2)
    occ = rng.random((n, P, S)) * 0.6
    rgb = rng.random((n, P, S, 3))
    tn = np.where(hit, t[:, :, 0], np.inf)
    want = vo.composite(P, hit, t, occ, rgb, t_near=tn, with_sensitivity=True)
    got = so.composite(P, hit, list(t), list(occ), list(rgb), np.full(n, S), t_near=tn, with_sensitivity=True)
    for key in ("depth", "color", "opacity", "instance", "weights", "n_hits"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("depth", "color", "opacity"):
        assert np.array_equal(got["sensitivity"][key], want["sensitivity"][key]), key
    assert np.array_equal(got["n_terms"], hit.sum(0) * S)
    # object 2 with 4 samples only
    S_obj = np.array([S, S, 4, S, S])
    cut = lambda a: [a[k][:, :S_obj[k]] for k in range(n)]
    got = so.composite(P, hit, cut(t), cut(occ), cut(rgb), S_obj, t_near=tn)
    t2, occ2 = t.copy(), occ.copy()
    t2[2, :, 4:], occ2[2, :, 4:] = 1e9, 0.0
    want = vo.composite(P, hit, t2, occ2, rgb, t_near=tn)
    for key in ("depth", "color", "opacity", "instance"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["n_terms"], (hit * S_obj[:, None]).sum(0))
