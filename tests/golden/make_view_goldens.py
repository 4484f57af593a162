"""Record the bits of the view renderer: tests/golden/view_bits.npz, which tests/test_gpu_view_bits.py compares every later build with.

Needs the GPU and the built package.  Only the public API of ``vmap_amd.render`` is used (``render_view``, ``render_view_groups``,
``FieldGroup``), on the scenes the GPU tests build (tests/view_oracle.py ``Standard``, the centres and the room of
tests/test_gpu_scene_view.py), so the script runs unchanged on any commit that has that API.  ``cases()`` is what the test calls too: one
definition of the inputs.

Every array is stored as its bits (floats as uint32).  An array of more than ``FULL_BYTES`` - the per-sample occupancy and colour
buffers - is stored as the SHA-256 of those bits and its shape (keys ``<case>/<name>/sha256`` and ``/shape``): equal digests are equal
bits, and the fixture stays under the size limit of a committed file.

    python tests/golden/make_view_goldens.py [OUT.npz]

The committed fixture was recorded at 61f6f4f, the last commit with the separate single-group kernels.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
sys.dont_write_bytecode = True

PATH = os.path.join(HERE, "view_bits.npz")
FULL_BYTES = 256 << 10
RANGE = (37, 5001)                          # begins and ends off a 64-pixel block
RANGE_BUDGET = 200_000                      # bytes of samples per call: the range is cut into at least three bands (asserted)


def bits(x):
    """The array's bits on the host: float32 as uint32 (so that -0.0 and NaN payloads count), everything else as it is."""
    x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def record(out, case, **arrays):
    for name, x in arrays.items():
        x = bits(x)
        if x.nbytes > FULL_BYTES:
            out[f"{case}/{name}/sha256"] = np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8)
            out[f"{case}/{name}/shape"] = np.asarray(x.shape, np.int64)
        else:
            out[f"{case}/{name}"] = x


def images(v):
    return dict(depth=v.depth, color=v.color, opacity=v.opacity, instance=v.instance)


def slabs():
    """The 20 slabs of test_more_than_sixteen_boxes_composite_the_nearest_sixteen and its thin-media parameter edit."""
    import view_oracle as vo
    return [vo.Box((0, 0, 1.0 + 0.2 * ((7 * k) % 20)), np.eye(3), ((0.4 if k >= 14 else 8.0), 8.0, 0.05)) for k in range(20)]


def thin(params):
    params[0][8] *= np.float32(0.1)
    params[0][9][:] = np.float32(-0.3)
    return params


def cases():
    """{key: bits} of every case, rendered now."""
    import torch
    import scene_view_oracle as so
    import view_oracle as vo
    from test_gpu_scene_view import CENTERS32, ROOM_CENTER
    from test_gpu_view import B3, stacked
    from vmap_amd import render, synth

    STD = vo.Standard
    out = {}
    T = vo.ring_pose(*STD.VIEWS[0])
    p32, p128 = synth.make_params(4, 32, seed=5), synth.make_params(1, 128, seed=6)
    std = (stacked(p32), [B3(b) for b in STD.boxes()], T, STD.k4(), STD.W, STD.H)
    kw = dict(samples=STD.S, min_depth=STD.MIN_DEPTH, centers=CENTERS32)

    v = render.render_view(*std, return_samples=True, **kw)
    assert v.n_pairs > 0 and v.sample_occ.shape == (v.n_pairs, STD.S)
    record(out, "std32", **images(v), overflow=np.int64(v.overflow), n_pairs=np.int64(v.n_pairs), pairs=v.pairs, offsets=v.offsets,
           sample_occ=v.sample_occ, sample_rgb=v.sample_rgb)

    v = render.render_view(*std, pixel_range=RANGE, budget_bytes=RANGE_BUDGET, **kw)
    assert v.bands >= 3, v.bands
    record(out, "std32_range", **images(v), n_pairs=np.int64(v.n_pairs), bands=np.int64(v.bands))

    eye, k4 = np.eye(4, dtype=np.float32), (30.0, 30.0, 11.5, 3.5)
    v = render.render_view(stacked(thin(synth.make_params(20, 32, seed=9))), [B3(b) for b in slabs()], eye, k4, 24, 8, samples=4, min_depth=0.05)
    assert v.overflow > 0
    record(out, "cap32", **images(v), overflow=np.int64(v.overflow))

    group = lambda params, boxes, centers, S: render.FieldGroup(stacked(params), [B3(b) for b in boxes], centers, S)
    v = render.render_view_groups([group(p32, STD.boxes(), CENTERS32, 16), group(p128, [so.ROOM], ROOM_CENTER, 48)], T, STD.k4(), STD.W, STD.H,
                                  min_depth=STD.MIN_DEPTH, return_samples=True)
    assert v.sample_occ.dim() == 1
    record(out, "mixed", **images(v), pairs=v.pairs, offsets=v.offsets, sample_occ=v.sample_occ, sample_rgb=v.sample_rgb)

    groups = [group(thin(synth.make_params(10, hidden, seed=9 + g)), slabs()[g::2], None, S) for g, (hidden, S) in enumerate(((32, 4), (64, 6)))]
    v = render.render_view_groups(groups, eye, k4, 24, 8, min_depth=0.05)
    assert v.overflow > 0
    record(out, "mixed_cap", **images(v), overflow=np.int64(v.overflow))
    torch.cuda.synchronize()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    out = cases()
    np.savez_compressed(path, **out)
    for k, x in out.items():
        print(f"{k:32s} {x.dtype} {tuple(x.shape)}")
    size = os.path.getsize(path)
    print(f"{len(out)} arrays -> {path}: {size / 1024:.0f} KiB")
    assert size < (1 << 20), "a committed file stays under 1 MiB"


if __name__ == "__main__":
    main()
