"""TEST INFRASTRUCTURE (numpy only): Philox4x32-10 on the host and the random numbers the two samplers draw from it.

* ``philox4x32_10``: plain Python integers, one tuple per round.  ``philox4x32_10_v``: the same function on uint64 numpy arrays.
  Both are held to the known-answer vectors published with Random123 by tests/test_philox.py.
* ``frame_randoms``: what ``frame_sample`` (vmap_amd/csrc/sample_kernels.h) draws for one object of one frame, in the layout of
  ``sampler_cases.draw_randoms`` - so ``oracle/sampler_oracle.py`` fed with it predicts the kernel's Philox mode.
* ``surface_randoms``: what ``surface_sample`` (vmap_amd/csrc/eval_kernels.h) draws for one set.

Counter layout of the ray sampler, key = (seed & 2^32-1, seed >> 32):

    output          counter.x     counter.y  counter.z       counter.w (stream)  words
    kf_ids[f]       frame slot f  object     frame counter   0                   x
    u_w, u_h        ray           object     frame counter   1                   x, y
    u_z[4q..4q+3]   ray           object     frame counter   2 + q               x, y, z, w
    g_z[4q..4q+3]   ray           object     frame counter   16 + q              Box-Muller of (x, y) and of (z, w)

Integers and uniforms are exact by construction (24 random bits in a float32).  The normals are computed in float64 and rounded to
float32 once: the kernel's differ from them by the error of the device's logf / sqrtf / cosf / sinf and of its float32 angle."""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
MUL0, MUL1 = 0xD2511F53, 0xCD9E8D57          # Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11
WEYL0, WEYL1 = 0x9E3779B9, 0xBB67AE85

STREAM_KF, STREAM_PIXEL, STREAM_UZ, STREAM_GZ = 0, 1, 2, 16


def philox4x32_10(counter, key):
    """Philox4x32-10 in plain integers: ten rounds of (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1,
    lo(M0 c0)), the key bumped by the Weyl constants after each.  Pinned to the Random123 known-answer vectors by
    tests/test_philox.py; independent of the kernels' copies in its structure (plain integers, one tuple per round)."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = MUL0 * c0, MUL1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + WEYL0) & M32, (k1 + WEYL1) & M32
    return c0, c1, c2, c3


def philox4x32_10_v(c0, c1, c2, c3, k0, k1):
    """The same function on arrays: every argument an integer or an integer array of 32-bit words (they broadcast); four uint64 arrays
    of 32-bit words come back.  A 32 x 32-bit product fits a uint64, so nothing here wraps."""
    m = np.uint64(M32)
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(a, dtype=np.uint64) & m for a in (c0, c1, c2, c3, k0, k1)])
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(MUL0) * c0, np.uint64(MUL1) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & m, (p0 >> s) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(WEYL0)) & m, (k1 + np.uint64(WEYL1)) & m
    return c0, c1, c2, c3


def u01(word):
    """float32 in [0, 1) from the top 24 bits of a 32-bit word: float32(word >> 8) * 2^-24, exact."""
    return (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def seed_key(seed):
    return int(seed) & M32, (int(seed) >> 32) & M32


def sampler_words(x, obj, frame_counter, stream, seed):
    """The four words of the ray sampler's draw at (x = ray or frame slot, object, frame counter, stream)."""
    k0, k1 = seed_key(seed)
    return philox4x32_10_v(x, obj, int(frame_counter) & M32, stream, k0, k1)


def box_muller(words):
    """float64 [..., 4] standard normals of four words: (x, y) -> radius * cos, radius * sin; (z, w) likewise; radius
    sqrt(-2 log(1 - u)), angle 2 pi u, u = u01(word) (1 - u is in (0, 1]: the logarithm is finite)."""
    u = [u01(w).astype(np.float64) for w in words]
    r0, r1 = np.sqrt(-2.0 * np.log(1.0 - u[0])), np.sqrt(-2.0 * np.log(1.0 - u[2]))
    t0, t1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1)


def counter_blocks(F, P, n1, n2):
    """Every draw of one object and frame as (output, stream, number of counter.x values 0 .. n - 1): what frame_randoms walks."""
    FP, S = F * P, n1 + n2
    return [("kf_ids", STREAM_KF, F), ("pixel", STREAM_PIXEL, FP)] + \
           [("u_z", STREAM_UZ + q, FP) for q in range((S + 3) // 4)] + [("g_z", STREAM_GZ + q, FP) for q in range((n2 + 3) // 4)]


def keyframe_ids(F, K, last2, obj, seed, frame_counter):
    """int64 [F]: min(int(u01 * K), K - 1) of stream 0 at the frame slot, the product in float32 as the kernel forms it.  With more
    than two keyframes the last two slots are the latest two keyframes (vmap.py:329-331); of a single slot, where the reference's
    randint(size=(n_frames - 2,)) has no answer, the latest one."""
    u = u01(sampler_words(np.arange(F), obj, frame_counter, STREAM_KF, seed)[0])
    kf = np.minimum((u * np.float32(K)).astype(np.int64), K - 1)
    if K > 2:
        for f in range(max(F - 2, 0), F):
            kf[f] = last2[f - (F - 2)]
    return kf


def frame_randoms(scene, k, seed, frame_counter):
    """The dict sampler_cases.draw_randoms returns, as frame_sample draws it for object ``k`` of a frame made of scenes shaped like
    ``scene``: kf_ids int64 [F], u_w / u_h float32 [F, P], u_z float32 [F*P, S], g_z float32 [F*P, n2]."""
    F, P, n1, n2, K = (scene[key] for key in ("F", "P", "n1", "n2", "K"))
    FP, S = F * P, n1 + n2
    out = dict(kf_ids=None, u_z=np.empty((FP, 4 * ((S + 3) // 4)), np.float32), g_z=np.empty((FP, 4 * ((n2 + 3) // 4)), np.float32))
    for name, stream, n in counter_blocks(F, P, n1, n2):
        if name == "kf_ids":
            out["kf_ids"] = keyframe_ids(F, K, scene["last2"], k, seed, frame_counter)
            continue
        w = sampler_words(np.arange(n), k, frame_counter, stream, seed)
        if name == "pixel":
            out["u_w"], out["u_h"] = u01(w[0]).reshape(F, P), u01(w[1]).reshape(F, P)
        elif name == "u_z":
            q = stream - STREAM_UZ
            out["u_z"][:, 4 * q:4 * q + 4] = np.stack([u01(x) for x in w], axis=-1)
        else:
            q = stream - STREAM_GZ
            out["g_z"][:, 4 * q:4 * q + 4] = box_muller(w).astype(np.float32)
    out["u_z"], out["g_z"] = np.ascontiguousarray(out["u_z"][:, :S]), np.ascontiguousarray(out["g_z"][:, :n2])
    return out


def surface_randoms(n, set_index, stream, seed):
    """(u0 float64 [n], r float32 [n, 2]) of surface_sample for the ``n`` points of set number ``set_index`` (set_base + the set's
    place in the call): counter (point within the set, set, stream, 0); u0 = the 53 bits (x << 21 | y >> 11) * 2^-53, r = u01(z), u01(w)."""
    k0, k1 = seed_key(seed)
    x, y, z, w = philox4x32_10_v(np.arange(n), set_index, stream, 0, k0, k1)
    u0 = ((x << np.uint64(21)) | (y >> np.uint64(11))).astype(np.float64) * 2.0 ** -53
    return u0, np.stack([u01(z), u01(w)], axis=-1)
