"""GPU tier: a plain ``bench.py`` run - the contract line, exactly --steps timed steps, and what --dump-outputs writes: the outputs
of the timed path after its last step, the same as the same frame calls give from the seeded inputs in another process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vmap_amd import layout, step, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    steps, warmup = 30, 7
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    cfg = synth.CONFIGS["replica_room0_vmap"]
    n, R, S, H = cfg["n_obj"], cfg["R"], cfg["S"], cfg["H"]
    assert j["metric"] == "training rays/sec (all objects) per step" and j["unit"] == "rays/s" and j["higher_is_better"] is True
    assert j["steps"] == steps and j["warmup"] == warmup and j["repeats"]["n"] == 1 and not j["full"]
    assert j["value"] == pytest.approx(n * R / (j["ms_per_step"] * 1e-3)) and j["dtype"].startswith("f32")
    assert "roofline" not in j and "cpu_baseline" not in j and "other_configs" not in j

    # the same frame calls in this process: the warm-up, then the timed steps in frame calls of iters_per_frame (20) steps
    dev = torch.device("cuda:0")
    fc, B, sc = synth.make_params(n, H, scale=cfg["scale"], seed=0)
    frame = synth.make_batch(n, R * 20, S, seed=1)
    tfc = [torch.from_numpy(a).to(dev) for a in fc]
    tB, tsc = torch.from_numpy(B).to(dev), torch.from_numpy(sc).to(dev)
    fargs = [torch.from_numpy(frame[k]).to(dev) for k in ("pcs", "z", "gt_depth", "gt_rgb", "sem", "depth_mask")]
    op = step.VmapStep(n, R, S, H, device=dev, max_steps=20)
    bound = op.bind(tfc, tB, tsc, *fargs, opt=step.FusedAdamWState(n, H, dev, lr=1e-3, weight_decay=0.013))
    for k in (warmup, 20, steps - 20):
        res = bound.train_steps(k)
    torch.cuda.synchronize()
    want = {"loss": res.loss[k - 1:k], "flags": res.flags[k - 1].float(), "pe_B_layer_weight": tB}
    for t, name in enumerate(layout.FC_NAMES):
        want[f"fc{t:02d}_{name.replace('.', '_')}"] = tfc[t]
    assert sorted(os.listdir(out)) == sorted(name + ".npy" for name in want)
    for name, t in want.items():
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32 and np.all(np.isfinite(got)), name
        assert np.array_equal(got, t.cpu().numpy()), name
