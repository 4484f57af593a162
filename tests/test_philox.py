"""The samplers' Philox mode, CPU tier.

1. tests/philox_ref.py (plain integers and vectorised numpy) against the known-answer vectors published with Random123.
2. frame_sample of vmap_amd/csrc/sample_kernels.h on the CPU executor, generating its own numbers, against oracle/sampler_oracle.py
   fed with philox_ref.frame_randoms - every output of every object, as strictly as the test mode is checked.
3. Statistics of the replica (which 2. ties to the kernel): deterministic, every bound six standard deviations of its statistic."""
import math

import numpy as np
import pytest

import philox_ref as pr
import sampler_checks as sck
import simlib

# ---- 1. known answers ---------------------------------------------------------------------------------------------------------------

KAT = [  # Random123 kat_vectors, philox4x32 10: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert pr.philox4x32_10(counter, key) == want
    got = pr.philox4x32_10_v(*[np.array([c]) for c in counter], *key)
    assert tuple(int(w[0]) for w in got) == want
    assert all(w.dtype == np.uint64 for w in got)


def test_philox_vectorised_equals_plain_integers():
    rng = np.random.default_rng(0)
    w = rng.integers(0, 2 ** 32, (10000, 6), dtype=np.uint64)
    w[:100] |= np.uint64(1 << 31)                                  # words >= 2^31 for certain, and the corners
    w[100], w[101] = 0, pr.M32
    assert (w >= 2 ** 31).mean() > 0.4
    got = np.stack(pr.philox4x32_10_v(*w.T), axis=1)
    for row, g in zip(w.tolist(), got.tolist()):
        assert pr.philox4x32_10(tuple(row[:4]), tuple(row[4:])) == tuple(g)


def test_u01_is_exact_and_below_one():
    assert pr.u01(0) == 0 and pr.u01(0xFF) == 0 and pr.u01(0x100) == np.float32(2.0 ** -24)
    assert pr.u01(pr.M32) == np.float32(1.0 - 2.0 ** -24) and pr.u01(pr.M32).dtype == np.float32


def _enumerate_counters(F, P, n1, n2):
    return np.concatenate([np.stack([np.arange(n), np.full(n, s)], 1) for _, s, n in pr.counter_blocks(F, P, n1, n2)])


def test_counters_of_one_object_and_frame_never_repeat():
    """Object and frame counter are fixed words of the counter, so a repeat is a repeat of (counter.x, stream).  The largest supported
    shape (F * P = 2^24 rays, S = 32, n_bins = 16): every block has a stream of its own and fewer than 2^32 values of counter.x, the
    u_z streams 2 .. 9 end below the normals' 16 .. 19.  A small shape with the same streams, counter by counter: F > P, so frame
    slots (stream 0) and rays (stream 1) share values of counter.x and only the stream keeps them apart."""
    blocks = pr.counter_blocks(4096, 4096, 16, 16)
    streams = [s for _, s, _ in blocks]
    assert len(set(streams)) == len(streams) == 14 and all(0 < n <= 2 ** 24 for _, _, n in blocks)
    assert sorted(streams) == [0, 1] + list(range(2, 10)) + list(range(16, 20))
    c = _enumerate_counters(40, 7, 16, 16)
    assert len(c) == 40 + 280 * 13 and len(np.unique(c, axis=0)) == len(c)
    assert len(np.unique(c[:, 0])) == 280                          # ... and not by counter.x alone
    # what frame_randoms returns is drawn from exactly these blocks: a part-used last quad still costs a whole counter
    assert [b[1] for b in pr.counter_blocks(3, 5, 1, 2)] == [0, 1, 2, 16]
    assert [b[1] for b in pr.counter_blocks(3, 5, 4, 5)] == [0, 1, 2, 3, 4, 16, 17]


# ---- 2. exact replay on the CPU executor ---------------------------------------------------------------------------------------------
#
# obj3              three objects, one workgroup each: counter word 1 (the object) matters for k = 2
# bg_split4         nsplit = 4, seed (5 << 32) | 9, frame counter 0xFFFFFFFF: high key word, top of the counter range (+ 1 wraps to 0)
# twokf_split2      K = 2: no forced latest-two, every slot's keyframe comes from stream 0
# one_keyframe      K = 1
# all_slots_forced  K = 3, F = 2: both slots are the latest two keyframes
# S32               n1 = n2 = 16: all eight u_z streams and four normal streams, a sort without padding
# S3_257rays        n1 = 1, n2 = 2: a part-used u_z quad, 14 pads sort behind two values; F * P = 257: a second trip of the 256-thread loop
# ragged_split3     377 rays in three slices of 126, 126, 125
# shared_store      through the shared frame store (slots / inst)
# all_invalid       every sampled depth is 0 <= min_bound = 0.5: max_bound is a maximum over zeros
# one_slot          F = 1 with K = 4: the single slot is the latest keyframe (last2[1])

def _sample(scenes, nsplit, seed, c):
    return simlib.sim_sample(scenes, None, seed=seed, frame_counter=c & pr.M32, eps=sck.EPS, stop_eps=sck.STOP, nsplit=nsplit)


@pytest.mark.parametrize("case", sck.REPLAY_CASES)
def test_sim_sampler_philox_mode_equals_oracle_fed_with_the_replica(case):
    """Measured on the executor: the stratified cells of z (all but the surface normals' columns) equal the oracle's bit for bit, as
    they do in test mode; the normals' columns differ by at most 4.8e-7 in z and in pcs (obj3; 2.4e-7 for most cases): one unit in
    the last place of a depth above 4.  The bounds asserted are the test mode's, 3e-6 and 6e-6."""
    scenes, nsplit, seed, c = sck.replay_scenes(case)
    base = _sample(scenes, nsplit, seed, c)
    sck.check_replay(base, scenes, seed, c, exact_stratified=True)
    for s2, c2 in ((seed, c + 1), (seed + 1, c), (seed + 2 ** 32, c)):
        other = _sample(scenes, nsplit, s2, c2)
        assert (other["z"] != base["z"]).any(-1).mean() > 0.99, (s2, c2)
        sck.check_replay(other, scenes, s2, c2 & pr.M32, exact_stratified=True)


def test_sim_sampler_test_mode_stratified_cells_are_bit_equal():
    """The yardstick of the bit equality asked of the Philox mode above: test mode achieves it on the executor."""
    import sampler_cases
    for name in sampler_cases.CASES:
        sc = sampler_cases.build_scene(name)
        rnd = sampler_cases.draw_randoms(sc)
        out = simlib.sim_sample([sc], [rnd], eps=sck.EPS, stop_eps=sck.STOP)
        o = sck.oracle(sc, rnd)
        m = sck.stratified_cells(o, sc["n1"])
        assert 0.3 < m.mean() < 1 and np.array_equal(out["z"][0][m], o["z"][m])


def test_one_slot_takes_the_latest_keyframe():
    """F = 1 and more than two keyframes: pick_pixel's forced branch reads last2[1].  The reference has no answer there (its
    randint(size=(n_frames - 2,)) raises); the replica pins the kernel's: the newest keyframe."""
    scenes, _, seed, c = sck.replay_scenes("one_slot")
    sc = dict(scenes[0], last2=(1, 3))
    assert pr.frame_randoms(sc, 0, seed, c)["kf_ids"].tolist() == [3]
    assert pr.keyframe_ids(2, 4, (1, 3), 0, seed, c).tolist() == [1, 3]
    assert pr.keyframe_ids(5, 4, (1, 3), 0, seed, c).tolist()[3:] == [1, 3]
    out = _sample([sc], 0, seed, c)
    sck.check_replay(out, [sc], seed, c, exact_stratified=True)
    other = _sample([dict(sc, last2=(3, 1))], 0, seed, c)         # ... and it is last2[1] that is read, not last2[0]
    assert not np.array_equal(other["gt_depth"], out["gt_depth"])


def test_keyframe_clamp_is_never_reached():
    """pick_pixel clamps its keyframe to K - 1.  The largest uniform is 1 - 2^-24, and K (1 - 2^-24) lies strictly between K - ulp
    and K - ulp / 2 (exactly on K - ulp for a power of two), so the float32 product is below K for every K < 2^24: the clamp guards
    against another u01, not this one, and a kernel without it computes the same keyframes.  Pinned here on the replica's formula."""
    umax = pr.u01(pr.M32)
    K = np.concatenate([np.arange(1, 70000), 2 ** np.arange(17, 24), 2 ** np.arange(17, 24) + 1, [2 ** 24 - 1]]).astype(np.int64)
    assert ((umax * K.astype(np.float32)).astype(np.int64) == K - 1).all()


# ---- 3. statistics of the replica ----------------------------------------------------------------------------------------------------

SEED = 2024
N = 1 << 16                                                        # rays of the correlation and normal checks


def _corr(a, b):
    return float(np.corrcoef(np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel())[0, 1])


def test_replica_words_are_uniform():
    """256 bins of the top byte, 2^20 counters, each of the four words: chi-square with 255 degrees of freedom has mean 255 and
    variance 510; bound 255 +- 6 sqrt(510)."""
    n = 1 << 20
    for i, w in enumerate(pr.sampler_words(np.arange(n), 0, 0, pr.STREAM_PIXEL, SEED)):
        hist = np.bincount((w >> np.uint64(24)).astype(np.int64), minlength=256)
        chi2 = float(((hist - n / 256) ** 2).sum() / (n / 256))
        print(f"word {i}: chi2 = {chi2:.1f}")
        assert abs(chi2 - 255) < 6 * math.sqrt(510), (i, chi2)


def test_replica_draws_are_uncorrelated():
    """Sample correlation of N independent pairs has standard deviation 1 / sqrt(N): |r| < 6 / sqrt(N) for every pair."""
    bound = 6 / math.sqrt(N)
    sc = dict(F=N // 64, P=64, n1=16, n2=16, K=2, last2=(0, 1))
    a, b, nxt = pr.frame_randoms(sc, 3, SEED, 11), pr.frame_randoms(sc, 4, SEED, 11), pr.frame_randoms(sc, 3, SEED, 12)
    pairs = {"u_w ~ u_h": (a["u_w"], a["u_h"])}
    for j in range(31):                                            # the quad boundaries 3|4, 7|8, ... are streams apart
        pairs[f"u_z[{j}] ~ u_z[{j + 1}]"] = (a["u_z"][:, j], a["u_z"][:, j + 1])
    for key in ("u_w", "u_h", "u_z", "g_z"):
        pairs[f"{key}: object k ~ k + 1"] = (a[key], b[key])
        pairs[f"{key}: frame counter c ~ c + 1"] = (a[key], nxt[key])
    for j in range(16):
        pairs[f"u_z[{j}] ~ g_z[{j}]"] = (a["u_z"][:, j], a["g_z"][:, j])
        pairs[f"u_z[{16 + j}] ~ g_z[{j}]"] = (a["u_z"][:, 16 + j], a["g_z"][:, j])
    worst = max(pairs, key=lambda k: abs(_corr(*pairs[k])))
    print(f"{len(pairs)} pairs, worst |r| = {abs(_corr(*pairs[worst])):.5f} ({worst}), bound {bound:.5f}")
    for name, (x, y) in pairs.items():
        n = np.asarray(x).size
        assert abs(_corr(x, y)) < 6 / math.sqrt(n), name


def test_replica_normals_are_standard_normal():
    """N rays x 16 normals, n = 16 N values.  Mean: sd 1 / sqrt(n).  Variance: sd sqrt(2 / n).  Share beyond 3 sigma (what the clip
    at +- eps cuts, the scale being eps / 3): p = erfc(3 / sqrt 2), binomial sd sqrt(p (1 - p) / n).  Cos and sin member of a
    Box-Muller pair: correlation sd 1 / sqrt(pairs).  Six standard deviations each."""
    sc = dict(F=N // 64, P=64, n1=16, n2=16, K=2, last2=(0, 1))
    g = pr.frame_randoms(sc, 0, SEED, 0)["g_z"].astype(np.float64)
    n = g.size
    p = math.erfc(3 / math.sqrt(2))
    share = float((np.abs(g) > 3).mean())
    r = _corr(g[:, 0::2], g[:, 1::2])
    print(f"mean {g.mean():.5f} var {g.var():.5f} share beyond 3 sigma {share:.6f} (p = {p:.6f}) pair r {r:.5f}")
    assert np.isfinite(g).all()
    assert abs(g.mean()) < 6 / math.sqrt(n)
    assert abs(g.var() - 1) < 6 * math.sqrt(2 / n)
    assert abs(share - p) < 6 * math.sqrt(p * (1 - p) / n)
    assert abs(r) < 6 / math.sqrt(n // 2)
    for j in range(16):                                            # no column is the odd one out (a radius paired with another angle)
        assert abs(g[:, j].mean()) < 6 / math.sqrt(N) and abs(g[:, j].var() - 1) < 6 * math.sqrt(2 / N), j


def test_replica_keyframe_draw_covers_its_slots():
    """K = 7 keyframes, 70000 free frame slots (the last two are forced and left out): chi-square over the seven keyframes, 6 degrees
    of freedom, mean 6, variance 12, bound 6 +- 6 sqrt(12); keyframe K - 1 is reached, K never."""
    F, K = 70002, 7
    kf = pr.keyframe_ids(F, K, (5, 6), 0, SEED, 0)
    assert kf[-2:].tolist() == [5, 6]
    hist = np.bincount(kf[:-2], minlength=K + 1)
    chi2 = float(((hist[:K] - (F - 2) / K) ** 2).sum() / ((F - 2) / K))
    print(f"keyframe histogram {hist.tolist()} chi2 = {chi2:.2f}")
    assert hist[K] == 0 and hist[K - 1] > 0 and kf.min() == 0 and kf.max() == K - 1
    assert abs(chi2 - 6) < 6 * math.sqrt(12)
