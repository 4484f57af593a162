"""TEST INFRASTRUCTURE: the sampler's comparison against oracle/sampler_oracle.py, shared by tests/test_sampler.py (test mode, GPU
tier) and tests/test_philox.py (Philox mode replayed on the CPU executor), and the scenes of the replay cases."""
from __future__ import annotations

import numpy as np

import philox_ref
import sampler_cases
from oracle import sampler_oracle as so

EPS, STOP = 0.1, 0.05


def oracle(sc, rnd, eps=EPS, stop_eps=STOP):
    return so.sample_object(sc["rgbs"], sc["depth"], sc["t_wc"], sc["bbox"], rnd["kf_ids"], rnd["u_w"], rnd["u_h"], rnd["u_z"],
                            rnd["g_z"], sc["intr"], sc["center"], sc["n1"], sc["n2"], min_bound=sc["min_bound"], eps=eps, stop_eps=stop_eps)


def check_against_oracle(out, k, o):
    assert np.array_equal(out["sem"][k], o["labels"])
    assert np.array_equal(out["depth_mask"][k].astype(bool), o["valid"])
    assert np.array_equal(out["gt_depth"][k], o["depth"])
    assert np.abs(out["gt_rgb"][k] - o["rgb"].astype(np.float32) / np.float32(255.0)).max() < 1e-7
    assert np.abs(out["z"][k].astype(np.float64) - o["z"]).max() < 3e-6
    assert np.abs(out["pcs"][k].astype(np.float64) - o["pcs"]).max() < 6e-6


def stratified_cells(o, n1):
    """bool [F*P, S]: the cells of z that are stratified bins - uniforms only, no normals: every column of invalid-depth rays and of
    rays that do not hit this object, the first n1 columns of the rest."""
    m = np.ones(o["z"].shape, bool)
    m[np.ix_(o["valid"] & (o["labels"] == 1), np.arange(n1, o["z"].shape[1]))] = False
    return m


def replay_figures(out, scenes, seed, frame_counter):
    """-> (max |dz|, max |dpcs|, max |dz| over the stratified cells) of a Philox-mode frame against its replay; asserts nothing."""
    dz = dp = ds = 0.0
    for k, sc in enumerate(scenes):
        o = oracle(sc, philox_ref.frame_randoms(sc, k, seed, frame_counter))
        ez = np.abs(out["z"][k].astype(np.float64) - o["z"])
        dz, ds = max(dz, float(ez.max())), max(ds, float(ez[stratified_cells(o, sc["n1"])].max()))
        dp = max(dp, float(np.abs(out["pcs"][k].astype(np.float64) - o["pcs"]).max()))
    return dz, dp, ds


def check_replay(out, scenes, seed, frame_counter, exact_stratified=False):
    """Every object of a Philox-mode frame against the oracle fed with philox_ref.frame_randoms: check_against_oracle's tolerances,
    and the camera-to-surface bins of valid-depth rays bit for bit; ``exact_stratified``: every stratified cell of z bit for bit."""
    for k, sc in enumerate(scenes):
        o = oracle(sc, philox_ref.frame_randoms(sc, k, seed, frame_counter))
        check_against_oracle(out, k, o)
        z, valid = out["z"][k], o["valid"]
        assert np.array_equal(z[valid][:, :sc["n1"]], o["z"][valid][:, :sc["n1"]]), f"object {k}: camera-to-surface bins"
        if exact_stratified:
            strat = stratified_cells(o, sc["n1"])
            assert np.array_equal(z[strat], o["z"][strat]), f"object {k}: stratified bins"


def worst_normals(out, scenes, seed, frame_counter, bound=3e-6, limit=8):
    """The (u, angle) pairs behind the surface samples of z that miss ``bound``: [(object, ray, u, angle, |dz|)], for a report."""
    rows = []
    for k, sc in enumerate(scenes):
        o = oracle(sc, philox_ref.frame_randoms(sc, k, seed, frame_counter))
        bad = np.flatnonzero((np.abs(out["z"][k].astype(np.float64) - o["z"]) >= bound).any(1))
        for ray in bad[:limit]:
            for q in range((sc["n2"] + 3) // 4):
                w = philox_ref.sampler_words(np.array([ray]), k, frame_counter, philox_ref.STREAM_GZ + q, seed)
                u = [float(philox_ref.u01(x)[0]) for x in w]
                rows.append((k, int(ray), u[0], 2 * np.pi * u[1], float(np.abs(out["z"][k][ray].astype(np.float64) - o["z"][ray]).max())))
                rows.append((k, int(ray), u[2], 2 * np.pi * u[3], rows[-1][4]))
    return rows


# ---- the scenes of the replay cases: derived from sampler_cases' (whose names are bound to golden files) -----------------------------

def with_shape(sc, K=None, **over):
    """``sc`` with other F / P / n1 / n2 / min_bound ..., and with its first ``K`` keyframes only."""
    out = dict(sc, **over)
    if K is not None:
        out.update(K=K, last2=(K - 2, K - 1), **{key: sc[key][:K] for key in ("rgbs", "depth", "t_wc", "bbox")})
    return out


def distinct_objects(sc, n, seed=5):
    """n objects shaped like ``sc``: other centres and depths, so that what object k gets shows which object it was drawn for."""
    rng = np.random.default_rng(seed)
    return [sc] + [dict(sc, depth=np.where(sc["depth"] > 0, sc["depth"] + 0.1 * i, 0).astype(np.float32),
                        center=rng.uniform(-0.3, 0.3, 3).astype(np.float32)) for i in range(1, n)]


def replay_scenes(case):
    """-> (scenes of one frame, nsplit, seed, frame counter) of a replay case (tests/test_philox.py lists what each one reaches)."""
    B = sampler_cases.build_scene
    if case == "obj3":
        return distinct_objects(B("obj"), 3), 0, 7, 3
    if case == "bg_split4":
        return distinct_objects(B("bg"), 2), 4, (5 << 32) | 9, 0xFFFFFFFF
    if case == "twokf_split2":
        return distinct_objects(B("twokf"), 2), 2, 21, 0
    if case == "one_keyframe":
        return distinct_objects(with_shape(B("obj"), K=1), 2), 0, 3, 1
    if case == "all_slots_forced":
        return distinct_objects(with_shape(B("bg"), F=2), 2), 0, 4, 2
    if case == "S32":
        return distinct_objects(with_shape(B("obj"), n1=16, n2=16), 2), 0, 8, 5
    if case == "S3_257rays":
        return distinct_objects(with_shape(B("obj"), n1=1, n2=2, F=257, P=1), 2), 0, 9, 6
    if case == "ragged_split3":
        return distinct_objects(with_shape(B("obj"), F=13, P=29), 2), 3, 10, 7
    if case == "shared_store":
        from test_keyframes import _shared_scene
        return [_shared_scene(sc, 5 + i) for i, sc in enumerate(distinct_objects(B("obj"), 2))], 0, 11, 8
    if case == "all_invalid":
        sc = B("obj")
        return distinct_objects(with_shape(dict(sc, depth=np.zeros_like(sc["depth"])), min_bound=0.5), 2), 0, 12, 9
    if case == "one_slot":
        return distinct_objects(with_shape(B("obj"), F=1, P=6), 2), 0, 13, 10
    raise KeyError(case)


REPLAY_CASES = ("obj3", "bg_split4", "twokf_split2", "one_keyframe", "all_slots_forced", "S32", "S3_257rays", "ragged_split3",
                "shared_store", "all_invalid", "one_slot")
