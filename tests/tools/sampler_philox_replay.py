"""Measure the Philox mode of frame_sample on the device against its replay (tests/philox_ref.py + oracle/sampler_oracle.py): max |dz| and
|dpcs| per case of the GPU tier's replay tests (tests/test_sampler.py), with the (u, angle) pairs behind any surface sample that misses
the tests' 3e-6.  Asserts nothing: the tests do.

    python tests/tools/sampler_philox_replay.py --out profiles/sampler_philox_replay.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import sampler_cases  # noqa: E402
import sampler_checks as sck  # noqa: E402
import test_sampler as ts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["# Philox mode of frame_sample on an MI355X against its replay (tests/philox_ref.py + oracle/sampler_oracle.py)",
             "# bounds asserted by the tests: |dz| < 3e-6, |dpcs| < 6e-6; 'stratified' = the cells of z drawn from uniforms only",
             "# case                          split rays   max|dz|     max|dpcs|   max|dz| stratified"]
    bad = []

    def run(name, scenes, seed, c, **kw):
        smp = ts._device_sampler(scenes, seed, **kw)
        smp.frame_counter = c
        out = ts._host_frame(smp.sample())
        fig = sck.replay_figures(out, scenes, seed, c)
        lines.append(f"{name:32s}{str(kw.get('split', True)):6s}{str(kw.get('rays', False)):6s} {fig[0]:.3e}   {fig[1]:.3e}   {fig[2]:.3e}")
        print(lines[-1], flush=True)
        if fig[0] >= 3e-6:
            bad.append((name, kw, sck.worst_normals(out, scenes, seed, c)))

    for case in ("obj3", "S32", "S3_257rays"):
        scenes, _, seed, c = sck.replay_scenes(case)
        for split in (True, False):
            for rays in (False, True):
                run(case, scenes, seed, c, split=split, rays=rays)
    scenes, _, seed, _ = sck.replay_scenes("bg_split4")
    run("bg seed (5<<32)|9 frame 6", scenes, seed, 6)
    run("bg seed (5<<32)|9 frame 7", scenes, seed, 7)
    run("bg frame 200 x 120 = 24000 rays", [ts._bg_frame_scene()], 5, 1)
    rng = np.random.default_rng(21)
    twenty = []
    for i in range(20):
        sc = sampler_cases.build_scene("obj")
        twenty.append(dict(sc, depth=np.where(sc["depth"] > 0, sc["depth"] + 0.03 * i, 0).astype(np.float32),
                           center=rng.uniform(-0.3, 0.3, 3).astype(np.float32), seed=sc["seed"] + 7 * i))
    run("twenty objects", twenty, 5, 2, split=True)
    run("twenty objects", twenty, 5, 2, split=False)
    for name, kw, rows in bad:
        lines.append(f"# {name} {kw} exceeds 3e-6: (object, ray, u, angle, |dz|)")
        lines += [f"#   {r}" for r in rows]
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
