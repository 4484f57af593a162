"""bench.py - training rays/sec of the fused per-object step on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 200 --warmup 20
    python bench.py --gpus N --steps K --warmup W            (no launcher around it: starts its own N ranks, one per GPU, RCCL;
                                                              exit status 2 if the box has fewer than N devices)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W                (joins the launcher's ranks)

A "step" = one pass of the hot path over one synthetic batch already resident in HBM: encoding + field MLP
forward + compositing + loss + backward + fused AdamW for every object (train.py:293-326 without the data
plumbing).  Workload at N=1: BASELINE configs[1] (20 objects x 4-layer/32-hidden MLP, 120 rays/object, 10
samples/ray, fp32).  N>1: weak scaling - every rank owns its own 20 objects (objects are independent units,
no data-path collective); value = rays of all ranks / max-over-ranks time.

N>1 also trains the SHARED background model (train.py:308-316) ray-sharded over the ranks next to the objects - the path's
one real collective (ONE all-reduce of [gradients | loss terms] per step over RCCL) - and reports it under `with_background`;
`value` stays the objects-only rate (the metric).

A plain run sets up, pre-heats and warms up, times exactly --steps steps once and prints ONE JSON line (rank 0) with the contract
fields: metric, value, unit, higher_is_better, dtype, ms_per_step (+ the run's configuration).  --full adds everything else the
benchmark measures, each in runs of its own after the timed region (the timed region is then repeated --repeats times, default 5,
and the median reported):
  roofline     - the dominant kernel against the matrix peaks (fp32-equivalent and the executed bf16 pipe), timed live with the
                 dispatch's own begin / end events; HBM traffic observed by two rocprofv3 --pmc passes
  cpu_baseline / gpu_reference_baseline / gpu_eager_baseline - the reference's own step (oracle/_ref) on this host's cores and on
                 this GPU, and the eager ATen port (reported, not a target)
  value_fp32_equivalent_backward / value_exact_fp32_kernel / precision - the precision / throughput curve of the hidden-32 kernels
  other_configs / frame - the other BASELINE configurations and a whole mapping frame (N = 1)
  with_background / world.region_costs - the shared background model beside the objects and the region's collectives (N > 1)

--dump-outputs DIR writes what the timed path hands its caller after its last timed step - that step's loss and empty-mask
flags and the 15 trained parameter tensors of rank 0's objects - as DIR/<name>.npy (float32).  Inputs and initial parameters
come from fixed seeds and the pre-heat's training is undone before the warm-up, so the same arguments give the same inputs and
the same number of training steps in every run: two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from vmap_amd import layout, step, synth

FP32_MFMA_PEAK_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2500.0   # dense (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0
PREHEAT_MS_DEFAULT = 100.0


def _reference_runner():
    """oracle.ref_runner if the reference's own modules can be imported on this box (source tree, or oracle/_ref = the same four
    files byte-compiled by oracle/make_ref.py), else None.  Baseline legs only - never on the product path."""
    try:
        from oracle import ref_runner
        return ref_runner if ref_runner.reference_available() else None
    except Exception:
        return None


def cpu_baseline(cfg, budget_s=18.0):
    """The REFERENCE's own step (functorch vmap of its model.py / embedding.py, its loss.py / render_rays.py, torch.optim.AdamW:
    utils.py:30-34 + train.py:293-326, through oracle.ref_runner.ReferenceTrainer) on this host's cores; ~budget_s of CPU work in
    total.  ``kind`` "reference".  Where the reference cannot be imported (no oracle/_ref): the ATen port of the oracle, ``kind``
    "port".  The step is ~400 small ATen ops, so it does not scale with the core count: a few thread counts are tried, best kept."""
    ncpu = os.cpu_count() or 1
    fc, B, sc = synth.make_params(cfg["n_obj"], cfg["H"], scale=cfg["scale"], seed=0)
    batch = synth.make_batch(cfg["n_obj"], cfg["R"], cfg["S"], seed=1)
    rays = cfg["n_obj"] * cfg["R"]
    rr = _reference_runner()
    best = None
    cands = sorted({min(ncpu, t) for t in (8, 16, 32)})
    for threads in cands:
        torch.set_num_threads(threads)
        if rr is not None:
            tr = rr.ReferenceTrainer(fc, B, sc, cfg["H"], device="cpu")
            b = tr.to_device(batch)
            kind, what = "reference", f"the reference's own modules ({rr.SOURCE}): functorch vmap + loss.step_batch_loss + torch.optim.AdamW"
        else:
            from oracle import vmap_oracle_torch as vt          # checker/baseline only - never on the product path
            tr, b = vt.CpuTrainer(fc, B, sc), batch
            kind, what = "port", "ATen port of the oracle (oracle/vmap_oracle_torch.py; the reference could not be imported here)"
        for _ in range(2):
            tr.step(b)
        t0 = time.perf_counter()
        n = 0
        while True:
            tr.step(b)
            n += 1
            el = time.perf_counter() - t0
            if el > budget_s / len(cands) or n >= 1000:
                break
        r = {"value": rays * n / el, "unit": "rays/s", "cores": threads, "kind": kind, "ms_per_step": el / n * 1e3,
             "sample": f"{n} full steps (fwd+loss+bwd+AdamW) of the same workload, {what}, torch {torch.__version__} CPU "
                       f"{threads} threads of {ncpu} host CPUs, {el / n * 1e3:.2f} ms/step"}
        if best is None or r["value"] > best["value"]:
            best = r
    return best


def gpu_reference_baseline(cfg, dev, budget_s=3.0):
    """The north star's denominator, measured live: the REFERENCE's own vectorised step (train.py:293-326 with
    ``training_strategy = "vmap"``: functorch vmap of its unmodified modules + torch.optim.AdamW, ``training_device = cuda:0``)
    on THIS GPU through PyTorch-ROCm, for ~budget_s.  None where the reference cannot be imported."""
    rr = _reference_runner()
    if rr is None:
        # say WHY the north star's denominator is missing (no source tree here and oracle/_ref absent / compiled by another Python)
        try:
            from oracle import make_ref
            why = make_ref.why_unavailable()
        except Exception as e:      # noqa: BLE001
            why = f"{type(e).__name__}: {e}"
        return {"error": f"the reference cannot be imported on this box: {why}"}
    fc, B, sc = synth.make_params(cfg["n_obj"], cfg["H"], scale=cfg["scale"], seed=0)
    batch = synth.make_batch(cfg["n_obj"], cfg["R"], cfg["S"], seed=1)
    tr = rr.ReferenceTrainer(fc, B, sc, cfg["H"], device=dev)
    b = tr.to_device(batch)
    for _ in range(5):
        tr.step(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        for _ in range(10):
            tr.step(b)
        n += 10
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if el > budget_s or n >= 2000:
            break
    rays = cfg["n_obj"] * cfg["R"]
    return {"value": rays * n / el, "unit": "rays/s", "kind": "reference", "ms_per_step": el / n * 1e3,
            "sample": f"{n} steps of the reference's own vmap path ({rr.SOURCE}; functorch vmap + loss.step_batch_loss + backward + "
                      f"torch.optim.AdamW, incl. its host-synchronising mask checks) of the same workload on {torch.cuda.get_device_name(dev)}, "
                      f"torch {torch.__version__}"}


def gpu_eager_baseline(cfg, dev, budget_s=1.5):
    """The eager PyTorch-ROCm PORT of the step (oracle/vmap_oracle_torch.py: the same ATen ops without functorch) on THIS GPU:
    kept next to gpu_reference_baseline so that earlier rounds' figures stay comparable.  Baseline only."""
    from oracle import vmap_oracle_torch as vt          # baseline leg only - never on the product path
    fc, B, sc = synth.make_params(cfg["n_obj"], cfg["H"], scale=cfg["scale"], seed=0)
    batch = synth.make_batch(cfg["n_obj"], cfg["R"], cfg["S"], seed=1)
    tr = vt.CpuTrainer(fc, B, sc, device=dev)
    tb = {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}
    for _ in range(5):
        tr.step(tb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        for _ in range(10):
            tr.step(tb)
        n += 10
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if el > budget_s or n >= 2000:
            break
    rays = cfg["n_obj"] * cfg["R"]
    return {"value": rays * n / el, "unit": "rays/s", "kind": "port", "ms_per_step": el / n * 1e3,
            "sample": f"{n} eager steps (fwd+loss+bwd+torch.optim.AdamW) of the same workload on {torch.cuda.get_device_name(dev)}, "
                      f"torch {torch.__version__}"}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, res, k, tfc, tB):
    """--dump-outputs: what the timed path's caller holds after its last step, as float32 .npy files under ``dirname``: that step's
    loss (``loss`` [1]) and empty-mask switches (``flags`` [4]: drop_depth, drop_colour, drop_opacity, explode), and the trained
    parameters updated in place (``fc00_in_layer_0_weight`` .. ``fc13_out_color_bias`` [n, ...] in layout.FC_NAMES order,
    ``pe_B_layer_weight`` [n, 21, 3])."""
    arrays = {"loss": res.loss[k - 1:k], "flags": res.flags[k - 1].float()}
    for t, name in enumerate(layout.FC_NAMES):
        arrays[f"fc{t:02d}_{name.replace('.', '_')}"] = tfc[t]
    arrays["pe_B_layer_weight"] = tB
    arrays = {name: a.detach().cpu().numpy().astype(np.float32) for name, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"bench.py --dump-outputs: {total} bytes of outputs, more than {DUMP_LIMIT_BYTES}")
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def library_sha256():
    import hashlib
    from vmap_amd import _lib
    try:
        with open(_lib.LIB_PATH, "rb") as fh:
            return hashlib.sha256(fh.read()).hexdigest()
    except Exception:
        return None


def observe_traffic(config, weights, timeout_s=150):
    """HBM-side bytes per launch of the dominant kernel, OBSERVED for the library this process runs: two `rocprofv3 --kernel-trace --pmc`
    passes (FETCH_SIZE, WRITE_SIZE - one counter per pass, as MI355X_MICROARCH.md's HBM section prescribes) over tests/tools/run_steps.py of
    the same configuration, as subprocesses (counters cannot be sampled from inside this process); FETCH_SIZE doubled per the guide's
    gfx950 correction.  Returns (bytes per launch, note) or (None, why not)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    tool = os.path.join(ROOT, "tests", "tools", "run_steps.py")
    means = {}
    work = tempfile.mkdtemp(prefix="vmap_pmc_", dir="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(work, counter)
            r = subprocess.run([exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "-o", "p", "--",
                                sys.executable, tool, config, "40", weights], cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"),
                               stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s)
            vals = []
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if "step_main" in row["Kernel_Name"] and row["Counter_Name"] == counter:
                        vals.append(float(row["Counter_Value"]))
            if r.returncode != 0 or not vals:
                return None, f"{counter} pass: rc {r.returncode}, {len(vals)} dispatches"
            means[counter] = sum(vals) / len(vals)
        return (2.0 * means["FETCH_SIZE"] + means["WRITE_SIZE"]) * 1024.0, \
            (f"OBSERVED in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over tests/tools/run_steps.py {config} 40 {weights} "
             f"as subprocesses on the library this process loaded; mean per dispatch of the dominant kernel: FETCH {means['FETCH_SIZE']:.1f} KiB x 2 "
             f"(gfx950 correction, MI355X_MICROARCH.md) + WRITE {means['WRITE_SIZE']:.1f} KiB")
    except Exception as e:
        return None, f"{type(e).__name__}: {e}"
    finally:
        shutil.rmtree(work, ignore_errors=True)


def mfma_per_tile(H, weights_f32=True):
    """Matrix instructions (v_mfma_f32_32x32x16_bf16) one 32-point tile costs on the bf16-pipe kernels, from the kernels' structure:
    (output block, 16-deep step) pairs of the five layers - in 6, mid1 H/16, cat (H + 96)/16, mid2 H/16, colour (H + 48)/16 steps, H/32
    blocks each - times the products per pair (float32 weights: 6 forward + 3 d-prop + 3 weight-gradient; bf16 weights: 3 + 2 + 3),
    plus the ones-column bias gradients of mid1 / mid2 (4 per block) and the B_layer gradient unit (6).  Cross-checked against the
    hardware counters: 290 vs 288 measured per tile at hidden 32 (profiles/round4a_*), 2294 vs 2370 at hidden 128 (r02j / r04g)."""
    nb = H // 32
    pairs = nb * (6 + H // 16 + (H + 96) // 16 + H // 16 + (H + 48) // 16)
    return pairs * (12 if weights_f32 else 8) + 2 * nb * 4 + 6


def _median(xs):
    xs = sorted(xs)
    m = len(xs) // 2
    return xs[m] if len(xs) % 2 else 0.5 * (xs[m - 1] + xs[m])


def other_config_leg(name, weights, dev, ipf, steps=40, repeats=3, warmup=20, rays=False):
    """One of the OTHER BASELINE configurations (or the background step) measured like `value`: synthetic frame resident in HBM, bound
    frame calls, `steps` steps between synchronisations, median of `repeats`; the dominant kernel's own dispatch time from
    vmapstep_profile_train_steps.  Reported under `other_configs`; never part of `value`."""
    cfg = synth.CONFIGS[name]
    n, R, S, H = cfg["n_obj"], cfg["R"], cfg["S"], cfg["H"]
    fc, B, sc = synth.make_params(n, H, scale=cfg["scale"], seed=5)
    frame = synth.make_batch(n, R * ipf, S, seed=6)
    tfc = [torch.from_numpy(a).to(dev) for a in fc]
    tB, tsc = torch.from_numpy(B).to(dev), torch.from_numpy(sc).to(dev)
    fr = tuple(torch.from_numpy(frame[k]).to(dev) for k in ("pcs", "z", "gt_depth", "gt_rgb", "sem", "depth_mask"))
    if rays:
        # the frame handed over as rays (ABI v7, what sampler.FrameSampler(rays=True) emits): origin / direction per ray + object centres
        # instead of the points tensor - 24 + 4 S instead of 16 S bytes per ray; the kernels rebuild the points bit-identically
        rng = np.random.default_rng(7)
        o = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, R * ipf, 3)).astype(np.float32)).to(dev)
        d = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, R * ipf, 3)).astype(np.float32)).to(dev)
        c = torch.from_numpy(rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)).to(dev)
        fr = (step.RayPoints(o, d, c),) + fr[1:]
    op = step.VmapStep(n, R, S, H, device=dev, max_steps=ipf, weights=weights)
    opt = step.FusedAdamWState(n, H, dev, lr=1e-3, weight_decay=0.013)
    bound = op.bind(tfc, tB, tsc, *fr, opt=opt)

    def run(k):
        done = 0
        while done < k:
            j = min(ipf, k - done); bound.train_steps(j); done += j

    run(warmup)
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / steps * 1e3)
    ms = _median(ts)
    k_ms, _ = op.profile_train_steps(tfc, tB, tsc, *fr, opt=opt, n_steps=ipf)
    plan = op.plan()
    flops = layout.step_flops(n, R, S, H)
    out = {"workload": f"{name}: {n} objects x 4-layer/{H}-hidden MLP, {R} rays/object, {S} samples/ray, {weights} weights, fwd+loss+bwd+fused AdamW"
                       + (", sample points handed over as rays (origin, direction, z: ABI v7)" if rays else ""),
           "sample_bytes_per_ray": (24 + 4 * S + 18) if rays else (16 * S + 18),
           "ms_per_step": ms, "ms_per_step_repeats": ts, "rays_per_s": n * R / (ms * 1e-3), "kernel": plan["kernel"], "kernel_ms": k_ms,
           "frac": flops / (k_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, "frac_is": "fp32-equivalent (algorithmic FLOPs / kernel time / 157.3 TFLOP/s)",
           "plan": plan}
    if plan["kernel"] != "step_main_h32" and plan["kernel"] != "step_main_gen":
        tiles = {"step_main_s32": 4}.get(plan["kernel"], plan["tiles_per_round"] or 2)      # 32-point tiles per round / pass
        mm = n * plan["rounds_per_object"] * tiles * mfma_per_tile(H, weights == "f32")
        out["frac_of_executed_pipe"] = mm * 32768 / (k_ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS
        out["matrix_instructions_per_launch"] = mm
    return out


def precision_leg(dev):
    """The precision / throughput trade of the hidden-32 kernels as MEASURED errors against the reference's own 20-step frame
    (fixture tests/golden/cfg2_frame20.npz: the reference's loop on the headline shape, generated by tests/golden/make_frame_goldens.py):
    for the default kernel (bf16 matrix pipe: 6 split products forward, 3 backward) and the exact-fp32 kernel, the worst relative error
    of the per-step loss over the 20 steps and of the 15 first-step gradient tensors (max|a - b| / max|b| per tensor)."""
    from vmap_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import cases
    finally:
        sys.path.pop(0)
    c = cases.build_frame_case("cfg2_frame20")
    g = np.load(os.path.join(ROOT, "tests", "golden", "cfg2_frame20.npz"))
    n, R, S, H, steps = c["n"], c["R"], c["S"], c["H"], c["n_steps"]
    keys = ("pcs", "z", "gt_depth", "gt_rgb", "sem", "depth_mask")
    fr = tuple(torch.from_numpy(c["frame"][k]).to(dev) for k in keys)
    out = {"fixture": "tests/golden/cfg2_frame20.npz (the reference's own step loop, train.py:270-326, 20 steps x 20 objects x 120 rays)",
           "error_is": "max over the 20 steps of |loss - ref| / |ref|; max over the 15 tensors of max|g - ref| / max|ref| for step 0; the same for "
                       "the single-step fixture tests/golden/cfg2.npz (same shape, the reference's own step on other seeds)"}
    for label, tuning in (("default_split_bf16_6fwd_3bwd", None), ("split_bf16_6fwd_6bwd", {"kernel": _lib.KERNEL_S32_BWD6}),
                          ("exact_fp32_kernel", {"kernel": _lib.KERNEL_H32_F32})):
        fc = [torch.from_numpy(a).to(dev) for a in c["fc"]]
        B, sc = torch.from_numpy(c["B"]).to(dev), torch.from_numpy(c["scale"]).to(dev)
        op = step.VmapStep(n, R, S, H, device=dev, max_steps=steps, tuning=tuning)
        gfc, gB = [torch.zeros_like(t) for t in fc], torch.zeros_like(B)
        op.fwd_bwd(fc, B, sc, *(x[:, :R] for x in fr), grads_fc=gfc, grad_B=gB)
        gerr = 0.0
        for t in range(15):
            ref = g[f"g0_fc{t}" if t < 14 else "g0_B"].astype(np.float64)
            got = (gfc[t] if t < 14 else gB).cpu().numpy().astype(np.float64)[g["keep"]]
            gerr = max(gerr, float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)))
        res = op.train_steps(fc, B, sc, *fr, opt=step.FusedAdamWState(n, H, dev, lr=1e-3, weight_decay=0.013), n_steps=steps, ray_step=R)
        losses = res.loss.cpu().numpy().astype(np.float64)
        out[label] = {"loss_rel_err_max_over_steps": float((np.abs(losses - g["losses"]) / np.abs(g["losses"])).max()),
                      "grad_rel_err_step0_max_over_tensors": gerr}
        # the same kernels on the single-step fixture of the same shape (tests/golden/cfg2.npz): no ReLU unit of it sits inside the
        # forward's rounding, so this figure shows the BACKWARD's arithmetic (the frame's step 0 above holds one such unit for the
        # bf16-pipe forward - 1.7e-5 on one tensor whatever the backward does; the tests account for it unit by unit, conftest.kink_aware)
        c1, g1 = cases.build_case("cfg2"), np.load(os.path.join(ROOT, "tests", "golden", "cfg2.npz"))
        fc1 = [torch.from_numpy(a).to(dev) for a in c1["fc"]]
        B1, sc1 = torch.from_numpy(c1["B"]).to(dev), torch.from_numpy(c1["scale"]).to(dev)
        b1 = tuple(torch.from_numpy(c1["batch"][k]).to(dev) for k in keys)
        op1 = step.VmapStep(c1["n"], c1["R"], c1["S"], c1["H"], device=dev, tuning=tuning)
        gfc1, gB1 = [torch.zeros_like(t) for t in fc1], torch.zeros_like(B1)
        op1.fwd_bwd(fc1, B1, sc1, *b1, grads_fc=gfc1, grad_B=gB1)
        errs = [float(np.abs((gfc1[t] if t < 14 else gB1).cpu().numpy().astype(np.float64) - g1[f"g_fc{t}" if t < 14 else "g_B"]).max()
                      / (np.abs(g1[f"g_fc{t}" if t < 14 else "g_B"]).max() + 1e-30)) for t in range(15)]
        out[label]["grad_rel_err_single_step_fixture_max_over_tensors"] = max(errs)
        out[label]["grad_rel_err_single_step_fixture_median_over_tensors"] = float(np.median(errs))
    if "forloop_losses" in g.files:
        out["reference_vmap_vs_its_own_forloop_path"] = {"loss_rel_err_max_over_steps": float((np.abs(g["forloop_losses"] - g["losses"]) / np.abs(g["losses"])).max())}
    return out


def frame_leg(cfg, dev, ipf, obj_batch, reps=20):
    """One REAL mapping frame of the configuration (`do_bg: 1`, train.py:270-326 + :308-316): the object stack and the
    hidden-128 background model (1200 rays x 14 samples) through ``driver.HipMapper.train_frame_with_background`` - frames bound
    once (no per-step Python), two streams, the caller's stream joins both.  Untimed in `value`; reported under `frame`."""
    from vmap_amd.driver import HipMapper
    from vmap_amd.trainer import SimpleConfig, Trainer
    bcfg = synth.CONFIGS["background"]
    m = HipMapper(SimpleConfig(training_device=str(dev), n_iter_per_frame=ipf), device=dev)
    torch.manual_seed(3)
    for _ in range(cfg["n_obj"]):
        m.add_object(Trainer(SimpleConfig(training_device=str(dev), hidden_feature_size=cfg["H"], obj_scale=cfg["scale"])))
    m.attach_background(Trainer(SimpleConfig(training_device=str(dev), hidden_feature_size=bcfg["H"], obj_scale=bcfg["scale"])),
                        bcfg["R"], bcfg["S"])
    bframe = synth.make_batch(1, bcfg["R"] * ipf, bcfg["S"], seed=77)
    bg_batch = tuple(torch.from_numpy(bframe[k]).to(dev) for k in ("pcs", "z", "gt_depth", "gt_rgb", "sem", "depth_mask"))

    def timed(fn):
        for _ in range(3):                           # first call: plain path; second: binds the buffers; third: bound
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    b = m.bg
    t_obj = timed(lambda: m.train_frame(*obj_batch))
    t_bg = timed(lambda: m._frame_call("bg", b["op"], b["views"], b["scale"], bg_batch, b["opt"], ipf, bcfg["R"]))
    t_two = timed(lambda: m.train_frame_with_background(obj_batch, bg_batch))
    rays = cfg["n_obj"] * cfg["R"]
    return {"what": f"one mapping frame = {ipf} steps of the {cfg['n_obj']} object fields (hidden {cfg['H']}) AND {ipf} steps of the background field "
                    f"(hidden {bcfg['H']}, {bcfg['R']} rays x {bcfg['S']} samples) on two streams, driver.HipMapper.train_frame_with_background, "
                    "frames bound once; host clock around whole frames; not part of `value`",
            "objects_ms_per_frame": t_obj, "background_ms_per_frame": t_bg, "two_streams_ms_per_frame": t_two,
            "ms_per_step": t_two / ipf, "object_rays_per_s": rays * ipf / (t_two * 1e-3),
            "object_plus_background_rays_per_s": (rays + bcfg["R"]) * ipf / (t_two * 1e-3),
            "background_plan": b["op"].plan()}


def background_legs(args, cfg, dev, rank, world, ipf, dist, run_objects, rays_per_step):
    """The shared background model (train.py:308-316; hidden 128, 1200 rays x 14 samples per step) trained NEXT TO the objects,
    both ways SURVEY.md 8(e) names, each on its own stream beside the objects' frame calls:
      ray_sharded    - parallel.SharedBackgroundHip: every rank 1/N of the rays, ONE all-reduce of [gradients | loss terms] per step
      owner_computes - parallel.OwnerBackgroundHip: rank 0 all the rays with the plain frame call, ONE slab broadcast per frame
    plus the collective of the first on its own (the measured counterpart of DESIGN.md section 4's prediction).  Every rank calls
    this (collectives inside); all ranks get the same numbers (MAX over ranks), rank 0 reports them."""
    import torch.distributed as td
    from vmap_amd import fields, parallel
    bcfg = synth.CONFIGS["background"]
    torch.manual_seed(7)                                              # the same replica on every rank
    bfc = fields.OccupancyMap(hidden_size=bcfg["H"])
    bfc.apply(fields.init_weights)
    bpe = fields.UniDirsEmbed(max_deg=5, scale=bcfg["scale"])
    bR = bcfg["R"] // world                                           # this rank's share of the background rays of a step
    bframe = synth.make_batch(1, bcfg["R"] * ipf, bcfg["S"], seed=77)
    keys = ("pcs", "z", "gt_depth", "gt_rgb", "sem", "depth_mask")
    idx = np.concatenate([np.arange(i * bcfg["R"] + rank, i * bcfg["R"] + bR * world, world) for i in range(ipf)])
    bloc = tuple(torch.from_numpy(np.ascontiguousarray(bframe[k][0][idx])).to(dev) for k in keys)
    bg_stream = torch.cuda.Stream(device=dev)
    cur = torch.cuda.current_stream(dev)

    def barrier():
        if dist:
            td.barrier()
        torch.cuda.synchronize()

    def timed(frame_fn, steps, warmup):
        """frame_fn(k): k steps of the leg; host clock between barriers, MAX over ranks -> ms per step"""
        done = 0
        while done < warmup:
            k = min(ipf, warmup - done); frame_fn(k); done += k
        barrier()
        t0 = time.perf_counter()
        done = 0
        while done < steps:
            k = min(ipf, steps - done); frame_fn(k); done += k
        barrier()
        el = time.perf_counter() - t0
        if dist:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            td.all_reduce(t, op=td.ReduceOp.MAX)
            el = float(t.item())
        return el / steps * 1e3

    def beside_objects(bg_frame):
        """objects on the current stream, the background frame on its own stream, joined per frame call.  The objects' frame call is
        ISSUED first: its one collective (the flag reduction) must not queue behind the background frame's collectives (one
        communicator: collectives run in issue order, the same on every rank)."""
        def fn(k):
            fork = torch.cuda.Event(); fork.record(cur)
            bg_stream.wait_event(fork)
            run_objects(k)
            with torch.cuda.stream(bg_stream):
                bg_frame(k)
                join = torch.cuda.Event(); join.record(bg_stream)
            cur.wait_event(join)
        return fn

    out = {"hidden": bcfg["H"], "rays_per_step_all_ranks": bR * world, "rays_per_step_this_rank": bR, "samples_per_ray": bcfg["S"]}
    steps, warm = args.steps, args.warmup
    # ---- ray-sharded replicas ----
    with torch.cuda.stream(bg_stream):
        # the default group for both stacks: ONE communicator, so collectives execute in the order every rank issues them
        bg = parallel.SharedBackgroundHip(bfc, bpe, bR, bcfg["S"], dev, max_steps=ipf)

    def sharded_frame(k):
        bg.prepare_frame(*bloc, n_steps=k)
        for i in range(k):
            bg.step_prepared(i)

    def alone(frame):
        def fn(k):
            with torch.cuda.stream(bg_stream):
                frame(k)
        return fn

    ms_alone = timed(alone(sharded_frame), steps, warm)
    ms_beside = timed(beside_objects(sharded_frame), steps, warm)
    # the step's collective on its own, on the same stream: K all-reduces of the same buffer between two events
    with torch.cuda.stream(bg_stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        K = 200
        for _ in range(20):
            if dist:
                td.all_reduce(bg.buf)
        e0.record(bg_stream)
        for _ in range(K):
            if dist:
                td.all_reduce(bg.buf)
        e1.record(bg_stream)
    barrier()
    ar_us = e0.elapsed_time(e1) / K * 1e3 if dist else 0.0
    out["ray_sharded"] = {
        "collectives": "per frame: one all_reduce(SUM) of the [steps, 4] mask counts; per step: ONE all_reduce(SUM) of "
                       f"[gradient slab | loss terms] = {bg.buf.numel() * 4} bytes between two launches (forward/backward; AdamW + image rewrite + global loss/flags)",
        "background_only_ms_per_step": ms_alone, "beside_objects_ms_per_step": ms_beside,
        "allreduce_alone_us": ar_us, "launch_chain_without_collective_us_predicted": {1: 111.0, 2: 78.5, 4: 66.1, 8: 57.1}.get(world),
        "predicted_ms_per_step_DESIGN_4": {1: 0.111, 2: 0.105, 4: 0.095, 8: "0.090-0.110"}.get(world),
        "object_rays_per_s": rays_per_step / (ms_beside * 1e-3),
        "object_plus_background_rays_per_s": (rays_per_step + bR * world) / (ms_beside * 1e-3),
        "plan": bg.op.plan()}
    # ---- owner-computes ----
    ball = tuple(torch.from_numpy(np.ascontiguousarray(bframe[k][0])).to(dev) for k in keys) if rank == 0 else (None,) * 6
    with torch.cuda.stream(bg_stream):
        own = parallel.OwnerBackgroundHip(bfc, bpe, bcfg["R"], bcfg["S"], dev, owner=0, max_steps=ipf)
    owner_frame = lambda k: own.train_frame(*ball, n_steps=k)
    ms_alone = timed(alone(owner_frame), steps, warm)
    ms_beside = timed(beside_objects(owner_frame), steps, warm)
    out["owner_computes"] = {
        "collectives": f"per frame: ONE broadcast of the [1, P] parameter slab = {own.slab.numel() * 4} bytes from rank 0; none on the step path",
        "background_only_ms_per_step": ms_alone, "beside_objects_ms_per_step": ms_beside,
        "object_rays_per_s": rays_per_step / (ms_beside * 1e-3),
        "object_plus_background_rays_per_s": (rays_per_step + bcfg["R"]) / (ms_beside * 1e-3),
        "plan": own.op.plan() if own.op is not None else None}
    # compatibility with earlier rounds' records: the ray-sharded leg's figures at the top level
    out.update({"ms_per_step": out["ray_sharded"]["beside_objects_ms_per_step"], "object_rays_per_s": out["ray_sharded"]["object_rays_per_s"],
                "object_plus_background_rays_per_s": out["ray_sharded"]["object_plus_background_rays_per_s"]})
    return out


class Watchdog:
    """The legs behind the scored measurement must not be able to lose it: if they have not finished within `seconds` (an RCCL
    hang in a path that no 8-GPU node has run yet), every rank leaves through here - rank 0 after printing the line it has."""

    def __init__(self, seconds, on_fire):
        import threading
        self.t = threading.Timer(seconds, on_fire)
        self.t.daemon = True
        self.t.start()

    def cancel(self):
        self.t.cancel()


def summarise(out):
    """A compact block of the figures the long line spreads over its legs, appended as the LAST key: a harness that keeps only the tail of
    stdout (the driver's record keeps ~5 000 characters) still shows every measured configuration, the baselines and the precision pair."""
    r3 = lambda x: None if x is None else float(f"{x:.4g}")
    s = {}
    g, p, c = out.get("gpu_reference_baseline") or {}, out.get("gpu_eager_baseline") or {}, out.get("cpu_baseline") or {}
    s["value_rays_per_s"], s["ms_per_step"] = r3(out.get("value")), r3(out.get("ms_per_step"))
    s["repeats_ms_per_step"] = [r3(x) for x in (out.get("repeats") or {}).get("ms_per_step", [])]
    s["kernel_ms"], s["frac"] = r3(out["roofline"].get("kernel_ms")), r3(out["roofline"].get("frac"))
    s["exact_fp32_kernel_rays_per_s"] = r3((out.get("value_exact_fp32_kernel") or {}).get("value"))
    s["six_product_backward_rays_per_s"] = r3((out.get("value_fp32_equivalent_backward") or {}).get("value"))
    s["reference_on_this_gpu_rays_per_s"], s["reference_on_this_gpu_ms_per_step"], s["vs_reference_on_this_gpu"] = r3(g.get("value")), r3(g.get("ms_per_step")), r3(g.get("speedup"))
    s["aten_port_on_this_gpu_rays_per_s"] = r3(p.get("value"))
    s["reference_on_host_cpu_rays_per_s"], s["host_threads"], s["cpu_baseline_kind"] = r3(c.get("value")), c.get("cores"), c.get("kind")
    pr = out.get("precision") or {}
    s["precision_loss_err_grad_err_frame_step0_grad_err_single_step_fixture"] = {k: [r3(v.get("loss_rel_err_max_over_steps")), r3(v.get("grad_rel_err_step0_max_over_tensors")), r3(v.get("grad_rel_err_single_step_fixture_max_over_tensors"))]
                                        for k, v in pr.items() if isinstance(v, dict) and "loss_rel_err_max_over_steps" in v}
    s["other_configs_ms_per_step_rays_per_s_frac"] = {k: ([r3(v.get("ms_per_step")), r3(v.get("rays_per_s")), r3(v.get("frac"))] if "error" not in v else v["error"][:60])
                                                      for k, v in (out.get("other_configs") or {}).items()}
    f = out.get("frame") or {}
    s["frame_ms_objects_background_two_streams"] = [r3(f.get("objects_ms_per_frame")), r3(f.get("background_ms_per_frame")), r3(f.get("two_streams_ms_per_frame"))]
    s["traffic_bytes_per_launch"] = r3(out["roofline"].get("traffic"))
    return s


def emit(out):
    if out.get("full"):                             # a plain line holds only the contract fields: nothing to summarise
        try:
            out.pop("summary", None)
            out["summary"] = summarise(out)         # last key of the line
        except Exception as e:
            out["summary"] = {"error": f"{type(e).__name__}: {e}"}
    # RCCL writes its banner through C stdio (buffered when stdout is a file): push it out first, the JSON line stays last
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    print(json.dumps(out), flush=True)


def multi_rank_region_costs(td, dev, run, barrier, ipf, rays_per_step, flags, reduce_flags, frames=10, repeats=3):
    """N > 1 only.  (i) the cost of the two collectives a timed region of ONE frame call contains besides the work - the frame's
    flag all-reduce (4 x steps int32, MAX) and a barrier - each measured alone, back to back on the current stream; (ii) the objects'
    rate over `frames` frame calls per repeat between barriers (MAX over ranks), where those fixed costs are < 1 % of the region."""
    cur = torch.cuda.current_stream(dev)
    K = 50
    for _ in range(5):
        reduce_flags(flags)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(cur)
    for _ in range(K):
        reduce_flags(flags)
    e1.record(cur)
    torch.cuda.synchronize()
    flag_us = e0.elapsed_time(e1) / K * 1e3
    barrier()
    t0 = time.perf_counter()
    for _ in range(20):
        td.barrier()
    torch.cuda.synchronize()
    barrier_us = (time.perf_counter() - t0) / 20 * 1e6
    ts = []
    for _ in range(repeats):
        barrier()
        t0 = time.perf_counter()
        run(frames * ipf)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        barrier()
    t = torch.tensor(ts + [flag_us, barrier_us], dtype=torch.float64, device=dev)
    td.all_reduce(t, op=td.ReduceOp.MAX)
    t = [float(x) for x in t.tolist()]
    el = _median(t[:repeats])
    return {"flag_allreduce_alone_us_per_frame": t[repeats], "barrier_alone_us": t[repeats + 1],
            "ten_frame_region": {"frames_per_repeat": frames, "steps_per_repeat": frames * ipf, "ms_per_step": el / (frames * ipf) * 1e3,
                                 "value": rays_per_step / (el / (frames * ipf)),
                                 "ms_per_step_repeats": [x / (frames * ipf) * 1e3 for x in t[:repeats]]},
            "note": "MAX over ranks; `value` of the line is the contract's region (exactly --steps steps); these figures show how much of it "
                    "is the frame's one collective and how the rate reads when the region is ten frame calls long"}


def launch_ranks(n_gpus, argv):
    """`python bench.py --gpus N` with N > 1 and no launcher environment (WORLD_SIZE unset): start the N ranks HERE - one process per
    GPU through torch.distributed.run (the same command line the module docstring shows, rendezvous on 127.0.0.1 and a free port),
    wait for them and hand their exit status on.  Rank 0's JSON line goes straight to this process's stdout.  Refuses (exit status 2,
    message on stderr) when the box has fewer than N devices instead of reporting a number for fewer ranks - except for the gloo dry
    run of the multi-rank plumbing (VMAP_BENCH_BACKEND=gloo), where ranks knowingly share devices."""
    import socket
    import subprocess
    backend = os.environ.get("VMAP_BENCH_BACKEND", "nccl")
    try:
        have = torch.cuda.device_count()
    except Exception:
        have = 0
    if have < 1 or (backend == "nccl" and have < n_gpus):
        print(f"bench.py --gpus {n_gpus}: this box exposes {have} GPU(s); a scaling run is one rank per GPU over RCCL - refusing to "
              f"run fewer ranks and report them as {n_gpus}" + ("" if have < 1 else " (VMAP_BENCH_BACKEND=gloo runs a dry run of the "
              "multi-rank plumbing with ranks sharing devices; its timings mean nothing)"), file=sys.stderr, flush=True)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL between processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n_gpus) // n_gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    print(f"[bench.py] launching {n_gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env, stdin=subprocess.DEVNULL).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--config", default="replica_room0_vmap", choices=list(synth.CONFIGS))
    ap.add_argument("--iters-per-frame", type=int, default=20)       # config: render.iters_per_frame
    ap.add_argument("--weights", default="f32", choices=["f32", "bf16"])   # bf16: BASELINE configs[3]/[4] (fp32 masters + accumulate)
    ap.add_argument("--kernel", default="auto", choices=["auto", "gen", "wide", "f32", "ws1", "wp"])   # measurement: hidden 128 / 256 kernels; f32 = hidden 32
                                                                                                 # on the exact-fp32 matrix instruction (step_main_h32)
    ap.add_argument("--ws-two-tile", action="store_true")           # measurement: step_main_ws never uses single-tile rounds (tuning.ws_flags = 1; A/B)
    ap.add_argument("--ws-flags", type=int, default=0)               # measurement: tuning.ws_flags as is (4 = never three-tile rounds: the round-2 plan)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--slab", action="store_true")                   # the 15 stacked tensors as views of one [n, P] slab (measurement;
                                                                     # default: separately allocated, utils.update_vmap's own layout)
    ap.add_argument("--profile-reps", type=int, default=200)
    ap.add_argument("--preheat-ms", type=float, default=PREHEAT_MS_DEFAULT)   # untimed device pre-heat in front of the warm-up (named in the JSON)
    ap.add_argument("--no-gpu-baseline", action="store_true")
    ap.add_argument("--with-background", action="store_true")      # also train the SHARED background model (train.py:308-316; hidden 128,
                                                                     # 1200 rays / step split over the ranks, ONE gradient all-reduce per
                                                                     # step) next to the objects, on a second stream; reported separately.
                                                                     # ON by default with --full whenever WORLD_SIZE > 1 (the scaling run exercises RCCL)
    ap.add_argument("--no-background", action="store_true")
    ap.add_argument("--pmc-file", default=None)                      # roofline.traffic from THIS file (tests/tools/pmc_summary.py output of the
                                                                     # FETCH_SIZE / WRITE_SIZE passes tests/tools/gpu_bench_with_pmc.sh ran just before,
                                                                     # over the same library) instead of the committed counter file
    ap.add_argument("--no-pmc", action="store_true")                # do not spawn the two rocprofv3 --pmc passes that observe roofline.traffic (N = 1)
    ap.add_argument("--bg-timeout", type=float, default=float(os.environ.get("VMAP_BENCH_BG_TIMEOUT", "120")))   # watchdog of the background legs (s)
    ap.add_argument("--no-frame", action="store_true")              # skip the N = 1 `frame` leg (objects + background on two streams)
    ap.add_argument("--timed-only", action="store_true")            # skip the roofline / baseline legs (for kernel traces of the timed region)
    ap.add_argument("--unbound", action="store_true")               # marshal the arguments on every frame call (VmapStep.train_steps)
    ap.add_argument("--graph", action="store_true")                 # measurement: the bound frame call replayed as a hipGraph (bit-identical; no gain: profiles/r03i)
    ap.add_argument("--repeats", type=int, default=None)            # the timed region (EXACTLY --steps steps between barrier + synchronize) is measured this many
                                                                     # times back to back; ms_per_step / value = the MEDIAN, min / max / all reported
                                                                     # (default: 1 in a plain run, 5 with --full)
    ap.add_argument("--full", action="store_true")                  # also run every leg beside the headline figure (roofline, baselines, precision,
                                                                     # other configurations, frame, background, collectives): see the module docstring
    ap.add_argument("--dump-outputs", metavar="DIR", default=None)   # write the timed path's outputs after its last timed step as DIR/<name>.npy
    ap.add_argument("--no-other-configs", action="store_true")      # skip the `other_configs` legs (configs[0], [3], [4] and the background step)
    ap.add_argument("--no-precision", action="store_true")          # skip the `precision` leg (measured errors of the two hidden-32 kernels)
    ap.add_argument("--pmc-timeout", type=float, default=60.0)      # per rocprofv3 --pmc pass of the traffic observation (it runs LAST, under a watchdog)
    args = ap.parse_args()

    if args.gpus < 1:
        raise SystemExit(f"bench.py: --gpus {args.gpus}")
    if args.steps < 1:
        raise SystemExit(f"bench.py: --steps {args.steps}")
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: no launcher set the rank environment up, so this process becomes the launcher
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} != WORLD_SIZE {world}")
    # VMAP_BENCH_FORCE_DIST=1 exercises the N>1 code path (process group, flag all-reduce, max-over-ranks timing) with a
    # single rank - the only way to run it on a 1-GPU box
    dist = world > 1 or os.environ.get("VMAP_BENCH_FORCE_DIST") == "1"
    # VMAP_BENCH_BACKEND=gloo: a dry run of the N > 1 code path on a box with fewer GPUs than ranks (RCCL refuses two ranks on one
    # device; gloo carries device tensors through the host) - ranks then share devices (local_rank modulo the device count).
    # Timings of such a run mean nothing; it exists to exercise the multi-rank plumbing of this file.
    backend = os.environ.get("VMAP_BENCH_BACKEND", "nccl")
    dev_index = local_rank % torch.cuda.device_count() if backend != "nccl" else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if dist:
        import torch.distributed as td
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:                                  # VMAP_BENCH_FORCE_DIST=1 without a launcher: a one-rank group
            for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_PORT", "29533")):
                os.environ.setdefault(k, v)
        if backend == "nccl":
            td.init_process_group("nccl", device_id=dev)
        else:
            td.init_process_group(backend)

    cfg = synth.CONFIGS[args.config]
    n, R, S, H = cfg["n_obj"], cfg["R"], cfg["S"], cfg["H"]
    ipf = args.iters_per_frame
    # every rank owns its own objects (weak scaling): different seeds per rank, same shapes
    fc, B, sc = synth.make_params(n, H, scale=cfg["scale"], seed=1000 * rank)
    frame = synth.make_batch(n, R * ipf, S, seed=1000 * rank + 1)        # [n, iters*R, ...] like train.py:255-260
    tfc = [torch.from_numpy(a).to(dev) for a in fc]
    tB, tsc = torch.from_numpy(B).to(dev), torch.from_numpy(sc).to(dev)
    if args.slab:
        # the stacked parameters as views of one [n, P] slab, the way vmap_amd.driver.HipMapper re-stacks an object list
        _, tfc, tB = layout.stack_in_slab(tfc, tB)
    fr = {k: torch.from_numpy(v).to(dev) for k, v in frame.items()}
    tuning = None
    if args.kernel != "auto":
        from vmap_amd import _lib
        tuning = {"kernel": {"gen": _lib.KERNEL_GEN, "wide": _lib.KERNEL_WIDE4, "f32": _lib.KERNEL_H32_F32, "ws1": _lib.KERNEL_WS1, "wp": _lib.KERNEL_WP}[args.kernel]}
    if args.ws_two_tile or args.ws_flags:
        tuning = dict(tuning or {}, ws_flags=(1 if args.ws_two_tile else 0) | args.ws_flags)
    op = step.VmapStep(n, R, S, H, device=dev, max_steps=ipf, weights=args.weights, tuning=tuning)
    opt = step.FusedAdamWState(n, H, dev, lr=1e-3, weight_decay=0.013)
    fargs = (fr["pcs"], fr["z"], fr["gt_depth"], fr["gt_rgb"], fr["sem"], fr["depth_mask"])

    flag_reduce = None
    if dist:
        # N-GPU == 1-GPU semantics: the batch-wide empty-mask switches are max-reduced once per frame (not per step)
        from vmap_amd import parallel
        flag_reduce = parallel.ObjectShard(n * world).reduce_flags

    # the frame tensors and the stacked parameters do not move between frame calls: marshal them once (BoundFrame), as
    # driver.HipMapper does for its slab and its sampler's frame buffers
    bound = None if args.unbound else op.bind(tfc, tB, tsc, *fargs, opt=opt, flag_reduce=flag_reduce, graph=args.graph)

    last = {}                                  # the last frame call's result and step count (--dump-outputs)

    def run(n_steps):
        done = 0
        while done < n_steps:
            k = min(ipf, n_steps - done)
            if bound is not None:
                res = bound.train_steps(k)
            else:
                res = op.train_steps(tfc, tB, tsc, *fargs, opt=opt, n_steps=k, flag_reduce=flag_reduce)
            done += k
        if n_steps > 0:
            last["res"], last["k"] = res, k

    def barrier():
        if dist:
            td.barrier()
        torch.cuda.synchronize()

    preheat_steps = 0
    if args.preheat_ms > 0:
        # Untimed device pre-heat (NOT part of the W warm-up steps and NOT timed): the same frame call repeated for
        # ~preheat_ms so that the clocks / power state are those of a running mapper rather than of an idle chip.
        # With several ranks every frame call contains a collective (the flag reduction), so the NUMBER of pre-heat frames must
        # be the same on every rank: it is fixed from a timed probe (MAX over ranks), not by each rank's own clock.
        # The number of pre-heat frames follows the clock, so the training it does is undone afterwards: the warm-up and the timed
        # region start from the seeded parameters and a fresh optimiser, whatever the pre-heat took (--dump-outputs compares runs).
        state = [t.clone() for t in tfc] + [tB.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()]
        if opt.step_counter is not None:                # --graph: the optimiser's step count lives on the device
            state.append(opt.step_counter.clone())
        step0 = opt.step
        run(ipf)
        torch.cuda.synchronize()
        t_ph = time.perf_counter()
        run(ipf)
        torch.cuda.synchronize()
        frames = max(1, int(np.ceil(args.preheat_ms * 1e-3 / max(time.perf_counter() - t_ph, 1e-6))))
        if dist:
            t = torch.tensor([frames], dtype=torch.int64, device=dev)
            td.all_reduce(t, op=td.ReduceOp.MAX)
            frames = int(t.item())
        frames = min(frames, 4000)
        for _ in range(frames):
            run(ipf)
        # in place: the bound frame holds these tensors' addresses
        live = list(tfc) + [tB, opt.exp_avg, opt.exp_avg_sq] + ([opt.step_counter] if opt.step_counter is not None else [])
        for dst, src in zip(live, state):
            dst.copy_(src)
        opt.step = step0
        torch.cuda.synchronize()
        preheat_steps = (frames + 2) * ipf
    run(args.warmup)
    # the timed region: EXACTLY args.steps steps between barrier + synchronize on both sides - measured args.repeats times back to
    # back (nothing else in between), MAX over ranks per repeat; the line reports the MEDIAN repeat (+ min / max / all)
    # Every rank's clock stops when ITS device has drained (torch.cuda.synchronize()), the closing barrier follows; the line takes
    # the MAX over ranks = the moment the last rank finished, counted from the common start.  (Stopping the clock behind the closing
    # barrier instead adds one RCCL barrier to a region that is ONE frame call at the driver's K = 20 - that figure is reported next
    # to it as `incl_closing_barrier`.)
    own_times, own_times_b = [], []
    for _ in range(max(1, args.repeats)):
        barrier()
        t0 = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        barrier()
        own_times.append(t1 - t0)
        own_times_b.append(time.perf_counter() - t0)
    times, times_b = list(own_times), list(own_times_b)
    if dist:
        t = torch.tensor(own_times + own_times_b, dtype=torch.float64, device=dev)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        t = [float(x) for x in t.tolist()]
        times, times_b = t[:len(own_times)], t[len(own_times):]
    if args.dump_outputs and rank == 0:
        # before anything else trains these parameters further
        dump_outputs(args.dump_outputs, last["res"], last["k"], tfc, tB)
    # N > 1: what the region's collectives cost on their own, and the same measurement over TEN frame calls per repeat (a barrier is
    # then < 1 % of the region): reported beside `value`, which stays EXACTLY --steps steps per the contract
    region = None
    if dist and args.full:
        region = multi_rank_region_costs(td, dev, run, barrier, ipf, n * R * world,
                                         flags=torch.zeros(ipf, 4, dtype=torch.int32, device=dev), reduce_flags=flag_reduce)
    elapsed = _median(times)
    elapsed_own = _median(own_times)
    ms_per_step = elapsed / args.steps * 1e3
    rays_per_step = n * R * world
    value = rays_per_step / (elapsed / args.steps)
    repeats_info = {"n": len(times), "ms_per_step": [x / args.steps * 1e3 for x in times], "ms_per_step_min": min(times) / args.steps * 1e3,
                    "ms_per_step_max": max(times) / args.steps * 1e3, "reported": "median",
                    "each": f"{args.steps} steps: barrier + torch.cuda.synchronize(), clock, the steps, torch.cuda.synchronize(), clock, barrier; MAX over ranks",
                    "ms_per_step_incl_closing_barrier": _median(times_b) / args.steps * 1e3}

    # every rank's own clock around the timed region (the line reports MAX over ranks as ms_per_step, per the contract)
    per_rank_ms = [ms_per_step]
    if dist:
        t = torch.zeros(world, dtype=torch.float64, device=dev)
        t[rank] = elapsed_own / args.steps * 1e3
        td.all_reduce(t, op=td.ReduceOp.SUM)
        per_rank_ms = [float(x) for x in t.tolist()]
    with_bg = None
    if args.timed_only:
        if dist:
            td.barrier()
            td.destroy_process_group()
        if rank == 0:
            try:
                import ctypes
                ctypes.CDLL(None).fflush(None)
            except Exception:
                pass
            print(json.dumps({"value": value, "ms_per_step": ms_per_step, "steps": args.steps, "warmup": args.warmup,
                              "preheat_ms": args.preheat_ms, "timed_only": True, "repeats": repeats_info}), flush=True)
        return
    # who took part (so that a scaling run can show its N ranks): device of every rank + the RCCL version torch links
    devices = [torch.cuda.get_device_name(dev) + f" (cuda:{dev_index})"]
    rccl_version = None
    if dist:
        gathered = [None] * world
        pr = torch.cuda.get_device_properties(dev)
        # a device's identity: its PCI address + UUID + index (two ranks on ONE device share all of them; two devices cannot share a PCI address)
        ident = (devices[0], "|".join(str(getattr(pr, k, "?")) for k in ("pci_domain_id", "pci_bus_id", "pci_device_id", "uuid")) + f"|cuda:{dev_index}")
        td.all_gather_object(gathered, ident)
        devices = [g[0] for g in gathered]
        try:
            rccl_version = ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception:
            rccl_version = None
        if backend == "nccl" and world > 1:
            # a scaling run is one rank per GPU over RCCL, nothing else: fail loudly instead of reporting a number for another setup
            if len({g[1] for g in gathered}) != world:
                raise SystemExit(f"bench.py --gpus {world}: ranks share devices {gathered}")
            if td.get_backend() != "nccl" or rccl_version is None:
                raise SystemExit(f"bench.py --gpus {world}: backend {td.get_backend()} / RCCL version {rccl_version}")
    out = None
    if rank == 0:
        # which kernel ran and how the batch was cut: asked from the library (vmapstep_describe_plan), not re-derived here
        plan = op.plan()
        pk = plan["kernel"]
        split = pk == "step_main_s32"
        wp = pk.startswith("step_main_wp")
        wsk = wp or pk.startswith("step_main_ws")
        ws8 = pk == "step_main_ws<8>"
        ws_nt = plan["tiles_per_round"] if pk.startswith("step_main_ws") else 2
        kernel_name = ("step_main_s32 (hidden 32: bf16 matrix pipe, split operands: 6 products forward, 3 backward)" if split else
                       "step_main_h32 (hidden 32: exact-fp32 matrix instruction)" if pk == "step_main_h32" else
                       (("step_main_wp" if wp else "step_main_ws") + f" (hidden {H}: bf16 matrix pipe, split operands, {('one', 'two', 'three')[ws_nt - 1]} 32-point "
                        f"tile{'s' if ws_nt > 1 else ''} per workgroup round, " + ("two waves" if wp else "one wave") + " per output block" + (", eight waves" if ws8 else "")
                        + (", one round per workgroup" if plan["single_round"] else f", {plan['rounds_per_object']} rounds on {plan['workgroups_per_object']} workgroups per object") + ")") if wsk else
                       pk + f" (hidden {H}: exact-fp32 matrix instruction)")
        on_bf16_pipe = split or wsk
        dtype_label = ("f32 I/O, masters, accumulation" + ("" if args.weights == "f32" else " on bf16-rounded run-time weights") +
                       ("; matrix operands split into bf16 planes: forward 6 products (~2^-24, float32-equivalent), backward 3 (~2^-16)"
                        if on_bf16_pipe and args.weights == "f32" else
                        "; bf16 matrix pipe: one weight plane x three activation planes forward, 2 + 3 products backward" if on_bf16_pipe
                        else "; exact-fp32 matrix instruction"))
        out = {
            "full": args.full,
            "metric": "training rays/sec (all objects) per step", "value": value, "unit": "rays/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "repeats": repeats_info,
            "dtype": dtype_label, "data": "synthetic",
            "config": {"workload": f"{args.config}: {n} objects/GPU x 4-layer/{H}-hidden MLP, {R} rays/object, "
                                   f"{S} samples/ray, fwd+loss+bwd+fused AdamW, {ipf} steps per frame call",
                       "objects_per_gpu": n, "rays_per_object": R, "samples_per_ray": S, "hidden": H,
                       "parallelism": f"objects sharded over {world} GPU(s); no per-step collective, one 4x{ipf}-int32 flag all-reduce per frame"},
            "preheat": {"ms": args.preheat_ms, "steps": preheat_steps, "timed": False},
            "world": {"world_size": world, "devices": devices, "rccl": rccl_version, "backend": backend if dist else None,
                      "ms_per_step_per_rank": per_rank_ms, "region_costs": region,
                      "weak_scaling_prediction": ("objects shard with no collective on the step path; per frame ONE all_reduce(MAX) of 4 x steps int32 (a ring of "
                                                  "latency-bound hops: 20-40 us at 8 ranks = 3-6 % of a 0.6 ms frame of 20 steps) => >= 7.5x at 8 GPUs expected against the "
                                                  "north star's >= 6x (DESIGN.md section 4); measured cost of that collective and of a barrier: region_costs") if world > 1 else None},
            "frame_call": ("marshalled per call" if bound is None else
                           "bound (arguments marshalled once), replayed as a hipGraph per frame (device-resident optimiser step count)" if bound.graph
                           else "bound (arguments marshalled once), launched kernel by kernel"),
        }
    if rank == 0 and args.full:
        # ---- dominant kernel, timed live on the launch stream ----
        # (event pairs around every launch of the dominant kernel inside the real prep / main / finalize sequence; `frac`
        # uses the RAW pair time, which is what a rocprofv3 --kernel-trace of the same command reports per dispatch
        # (profiles/); the time minus the cost of an empty event pair and back-to-back launches of the kernel alone are
        # reported next to it)
        b0 = tuple(x[:, :R] for x in fargs)
        k_ms_alone = op.profile_main_kernel(tfc, tB, tsc, *b0, reps=args.profile_reps)
        reps = max(1, args.profile_reps // ipf)
        pairs = [op.profile_train_steps(tfc, tB, tsc, *fargs, opt=opt, n_steps=ipf) for _ in range(reps)]
        k_ms = sum(p[0] for p in pairs) / reps               # the dispatch's own begin -> end timestamps (hipExtLaunchKernel events):
                                                             # the quantity a rocprofv3 --kernel-trace reports per dispatch (profiles/)
        k_ms_pair = sum(p[1] for p in pairs) / reps          # a pair of stream events around the launch (includes the events' own cost)
        flops = layout.step_flops(n, R, S, H)
        abytes = layout.step_bytes(n, R, S, H)
        achieved = flops / (k_ms * 1e-3) / 1e12
        # HBM-side bytes per launch from the committed rocprofv3 --pmc passes (FETCH_SIZE x2 + WRITE_SIZE, see
        # profiles/*_pmc_counters.json); counters cannot be sampled from inside this process
        traffic = None
        pmc_file = None
        try:
            # the committed counter file of the kernel this run used
            if args.config == "replica_room0_vmap" and split:
                pmc_file, key = "round6b_pmc_counters_step_main_s32.json", "hbm_traffic_bytes_per_launch_step_main"
            elif args.config == "replica_room0_vmap":
                pmc_file, key = "r01m_pmc_counters.json", "hbm_traffic_bytes_per_launch_step_main"
            elif args.config == "imap_plumbing" and ws8 and args.weights == "f32":
                pmc_file, key = "r04p_pmc_counters_imap_ws8.json", "hbm_traffic_bytes_per_launch_step_main_ws"
            elif args.config == "background" and args.kernel == "auto" and args.weights == "f32":
                # three-tile rounds (the automatic plan): r04g; the round-2 plan (--ws-flags 4): r03q
                pmc_file, key = ("round6b_pmc_counters_background_ws.json" if ws_nt == 3 else "r03q_pmc_counters_background_ws.json"), "hbm_traffic_bytes_per_launch_step_main_ws"
            if pmc_file:
                with open(os.path.join(ROOT, "profiles", pmc_file)) as fh:
                    traffic = json.load(fh)["_notes"][key]
        except Exception:
            traffic = None
        lib_sha = library_sha256()
        traffic_observed = None
        traffic_note = None
        # (the live observation - two rocprofv3 --pmc subprocess passes - runs LAST, under a watchdog, behind everything the scored
        # line needs: see the end of main(); until then `traffic` is the committed counter file's figure)
        if args.pmc_file:
            # counters taken in the same gpurun, by the script that also launched this process (tests/tools/gpu_bench_with_pmc.sh)
            with open(args.pmc_file) as fh:
                notes = json.load(fh)["_notes"]
            traffic = notes.get("hbm_traffic_bytes_per_launch_step_main")
            traffic_observed = {"file": args.pmc_file, "library_sha256_of_the_counter_passes": notes.get("library_sha256"),
                                "same_library": notes.get("library_sha256") == lib_sha, "workload": notes.get("workload")}
        # what the matrix pipe actually executes (bf16 kernels): instructions per 32-point tile / 64-point round x tiles x 32x32x16 x 2 FLOP
        executed_tflops, mm_per_launch = None, None
        if split:
            per_tile = 344 if args.weights == "f32" else 251      # 275.2 k matrix instructions per launch / 800 working waves (round6b counters); bf16 weights: 93 fewer
            mm_per_launch = n * ((R + (128 // S) - 1) // (128 // S)) * 4 * per_tile
        elif ws8 and args.weights == "f32":
            # 975 matrix instructions per wave and single-tile round (profiles/r04p_pmc_counters_imap_ws8.json), eight waves per round
            mm_per_launch = n * plan["rounds_per_object"] * 8 * 975
        elif wp:
            # step_main_wp: counted from the kernel's structure (mfma_per_tile: cross-checked against the counters of the other forms)
            mm_per_launch = n * plan["rounds_per_object"] * 2 * mfma_per_tile(H, args.weights == "f32")
        elif wsk and H == 128:
            gq = (32 * ws_nt) // S
            mm_per_launch = n * ((R + gq - 1) // gq) * 4 * (1285 if args.weights == "f32" else 907) * ws_nt // 2      # 1927 per wave and three-tile round (round6b counters)
        if mm_per_launch:
            executed_tflops = mm_per_launch * 32768 / (k_ms * 1e-3) / 1e12
        # Floor of THIS formulation at hidden 32 (one 32-point tile per wave, one wave per SIMD): a SIMD's time is the SUM of its matrix
        # and its vector instructions (measured: profiles/r02o_pair_probe.jsonl - neither a second wave nor interleaving overlaps
        # them): 296 matrix instructions x 32 clocks + 3838 vector instructions x 4.8 clocks = 27.9 k clocks at 2.4 GHz.
        floor_us, floor_note = None, None
        if split and args.weights == "f32":
            floor_us = (354 * 32 + 4505 * 4.8) / 2400.0
            floor_note = ("sum of one tile's matrix (354 x 32 clk) and vector (4505 x 4.8 clk; profiles/round6b_pmc_counters_step_main_s32.json) issue time on its SIMD at 2.4 GHz: the part of "
                          "kernel_ms no schedule of this tiling can remove; kernel_ms - floor_us = waits, barriers, issue stalls, launch ramp")
        if ws8 and args.weights == "f32":
            rounds_per_wg = -(-plan["rounds_per_object"] // plan["workgroups_per_object"])
            floor_us = rounds_per_wg * 2 * (975 * 32 + 3418 * 4.8) / 2400.0
            floor_note = (f"{rounds_per_wg} round(s) per workgroup x 2 waves per SIMD x (975 matrix x 32 clk + 3418 vector x 4.8 clk per wave and 32-point round, "
                          "hardware counters of this kernel form) at 2.4 GHz: issue time of the busiest SIMD only")
        if wsk and H == 128 and args.weights == "f32" and not wp:
            # the same sum for one 64-point round of step_main_ws (hardware counters, profiles/r02j_pmc_counters_background_ws.json:
            # 1185 matrix + 6149 vector instructions per wave and round), times the rounds the busiest workgroup runs
            nt = ws_nt
            rounds_per_wg = -(-plan["rounds_per_object"] // plan["workgroups_per_object"])
            if nt == 3:
                # the three-tile single-round form, counted afresh in round 6 (profiles/round6b_pmc_counters_background_ws.json): 1927 matrix
                # (on-pipe transposes included) + 8477 vector instructions per wave and 96-point round
                floor_us = rounds_per_wg * (1927 * 32 + 8477 * 4.8) / 2400.0
                floor_note = (f"{rounds_per_wg} round(s) per workgroup x (1927 matrix x 32 clk + 8477 vector x 4.8 clk per wave and 96-point round, hardware "
                              "counters of this kernel form) at 2.4 GHz: issue time only; the round's LDS and vector-memory phases run in between, not "
                              "underneath (DESIGN 3.1f)")
            else:
                floor_us = rounds_per_wg * (1185 * 32 + 6149 * 4.8) * (nt / 2.0) / 2400.0
                floor_note = (f"{rounds_per_wg} round(s) per workgroup x (1185 matrix x 32 clk + 6149 vector x 4.8 clk per wave and 64-point round"
                              + (f", x {nt}/2 for {nt}-tile rounds" if nt != 2 else "") + ") at 2.4 GHz: issue time only; the round's LDS (~38 k clk) and "
                              "vector-memory (~35-45 k clk) phases run in between, not underneath (DESIGN 3.1f)")
        # forward+backward only (no optimiser), same loop structure
        gfc = [torch.zeros_like(t) for t in tfc]
        gB = torch.zeros_like(tB)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(100):
            op.fwd_bwd(tfc, tB, tsc, *b0, grads_fc=gfc, grad_B=gB)
        torch.cuda.synchronize()
        fb_ms = (time.perf_counter() - t1) / 100 * 1e3
        # the same workload on the exact-fp32 matrix instruction (step_main_h32: every product an fp32 FMA; the A/B reference of the
        # default kernel's split-bf16 operands), timed like `value`: the number to quote if the backward's ~2^-16 operands are not wanted
        exact, bwd6 = None, None
        if split and world == 1:
            from vmap_amd import _lib as _l
            op_x = step.VmapStep(n, R, S, H, device=dev, max_steps=ipf, weights=args.weights, tuning={"kernel": _l.KERNEL_H32_F32})
            opt_x = step.FusedAdamWState(n, H, dev, lr=1e-3, weight_decay=0.013)
            xfc, xB = [t.clone() for t in tfc], tB.clone()
            bx = op_x.bind(xfc, xB, tsc, *fargs, opt=opt_x)
            for _ in range(max(1, args.warmup // ipf)):
                bx.train_steps(ipf)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            done = 0
            while done < args.steps:
                k = min(ipf, args.steps - done)
                bx.train_steps(k)
                done += k
            torch.cuda.synchronize()
            x_ms = (time.perf_counter() - t1) / args.steps * 1e3
            exact = {"value": n * R / (x_ms * 1e-3), "ms_per_step": x_ms, "kernel": "step_main_h32 (v_mfma_f32_32x32x2_f32)"}
            # ... and on the default kernel with the SIX-product backward (tuning.kernel = VMAPSTEP_KERNEL_S32_BWD6: hi.lo + lo.hi + mid.mid on
            # top of the three, ~2^-24 like the forward): the float32-equivalent form of the bf16-pipe kernel, timed the same way
            if args.weights == "f32":
                op_6 = step.VmapStep(n, R, S, H, device=dev, max_steps=ipf, weights=args.weights, tuning={"kernel": _l.KERNEL_S32_BWD6})
                opt_6 = step.FusedAdamWState(n, H, dev, lr=1e-3, weight_decay=0.013)
                b6 = op_6.bind([t.clone() for t in tfc], tB.clone(), tsc, *fargs, opt=opt_6)
                for _ in range(max(1, args.warmup // ipf)):
                    b6.train_steps(ipf)
                ts6 = []
                for _ in range(max(1, args.repeats)):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    done = 0
                    while done < args.steps:
                        k = min(ipf, args.steps - done)
                        b6.train_steps(k)
                        done += k
                    torch.cuda.synchronize()
                    ts6.append((time.perf_counter() - t1) / args.steps * 1e3)
                k6_ms, _ = op_6.profile_train_steps([t.clone() for t in tfc], tB.clone(), tsc, *fargs, opt=opt_6, n_steps=ipf)
                bwd6 = {"value": n * R / (_median(ts6) * 1e-3), "ms_per_step": _median(ts6), "ms_per_step_repeats": ts6, "kernel_ms": k6_ms,
                        "frac": flops / (k6_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                        "kernel": "step_main_s32<bwd6> (bf16 matrix pipe, split operands: 6 products forward AND backward, ~2^-24 both ways)"}
        if traffic_observed:
            traffic_source = ("OBSERVED in this gpurun: FETCH_SIZE / WRITE_SIZE passes (rocprofv3 --pmc, separate passes, FETCH doubled per MI355X_MICROARCH.md) over "
                              "the library this process loaded, folded by tests/tools/pmc_summary.py: " + json.dumps(traffic_observed))
        elif traffic is not None:
            traffic_source = ((traffic_note or "") + "copied from the committed rocprofv3 --pmc passes of this kernel (profiles/" + pmc_file +
                              ": separate FETCH_SIZE / WRITE_SIZE passes over tests/tools/run_steps.py, FETCH doubled per MI355X_MICROARCH.md), not observed in this run")
        else:
            traffic_source = traffic_note
        out.update({
            "roofline": {"bound": "mfma", "kernel": kernel_name, "achieved": achieved,
                         "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / FP32_MFMA_PEAK_TFLOPS,
                         "frac_is": "fp32-EQUIVALENT: algorithmic float32 FLOPs (n R S 6 H (4H + 220)) per launch / launch duration / the float32 "
                                    "matrix = vector peak (157.3 TFLOP/s) - the rate of the path's arithmetic type; comparable across rounds",
                         "frac_of_executed_pipe": (executed_tflops / BF16_MFMA_PEAK_TFLOPS) if executed_tflops else achieved / FP32_MFMA_PEAK_TFLOPS,
                         "executed_pipe": ({"instruction": "v_mfma_f32_32x32x16_bf16", "peak_tflops": BF16_MFMA_PEAK_TFLOPS,
                                            "executed_tflops": executed_tflops, "matrix_instructions_per_launch": mm_per_launch}
                                           if executed_tflops else {"instruction": "v_mfma_f32_32x32x2_f32", "peak_tflops": FP32_MFMA_PEAK_TFLOPS}),
                         "launch_plan": plan, "floor_us": floor_us, "floor_note": floor_note,
                         "traffic": traffic,
                         "traffic_source": traffic_source,
                         "library_sha256": lib_sha,
                         "kernel_ms": k_ms, "kernel_ms_stream_event_pair": k_ms_pair,
                         "kernel_ms_note": "kernel_ms = average of the dispatches' own begin -> end timestamps (events attached to the launch, "
                                           "hipExtLaunchKernel) over the real prep / main / finalize sequence = what rocprofv3 --kernel-trace reports "
                                           "(profiles/); kernel_ms_stream_event_pair = events recorded on the stream around the launch",
                         "kernel_ms_back_to_back": k_ms_alone, "algorithmic_flops_per_launch": flops,
                         "algorithmic_bytes_per_launch": abytes,
                         "hbm_achieved_GBs": abytes / (k_ms * 1e-3) / 1e9,
                         "hbm_frac": abytes / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
            "value_exact_fp32_kernel": exact,
            "value_fp32_equivalent_backward": bwd6,
            "fwd_bwd_only": {"ms_per_step_host_launched": fb_ms, "rays_per_s": n * R / (fb_ms * 1e-3)},
            "with_background": with_bg,
            "frame": None,
        })
    if dist:
        td.barrier()
    if rank == 0 and args.full:
        if world == 1 and not args.no_gpu_baseline:
            # the north star's ">= 5x the reference single-GPU PyTorch path": the reference's OWN vmap step on this GPU, timed live
            try:
                ref_gpu = gpu_reference_baseline(cfg, dev)
            except Exception as e:
                ref_gpu = {"error": f"{type(e).__name__}: {e}"}
            out["gpu_reference_baseline"] = ref_gpu
            if ref_gpu and "value" in ref_gpu:
                ref_gpu["speedup"] = value / ref_gpu["value"]
                # BASELINE.md holds no published number for this metric ("None"); its section 3 names THIS measurement - the unmodified
                # reference on 1 MI355X through PyTorch-ROCm - as the denominator of the north-star target, so that is what the ratio is
                out["vs_baseline"] = value / ref_gpu["value"]
                out["vs_baseline_is"] = ("value / gpu_reference_baseline.value: the reference's own functorch-vmap step (train.py:293-326, unmodified "
                                         "modules from oracle/_ref) on this same GPU through PyTorch-ROCm, measured in this run (BASELINE.md section 3 item 2; "
                                         "there is no published number for this metric); north-star target >= 5")
            out["gpu_eager_baseline"] = gpu_eager_baseline(cfg, dev)
            out["gpu_eager_baseline"]["speedup"] = value / out["gpu_eager_baseline"]["value"]
            out["gpu_eager_baseline"]["speedup_is"] = "against the eager PyTorch-ROCm PORT of the step (oracle/vmap_oracle_torch.py), not the reference's functorch path"
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(cfg)
            g = out.get("gpu_reference_baseline") or {}
            if "value" in g:
                # the same reference code on THIS GPU, next to its host-CPU figure (scalars: a harness that keeps only the contract objects
                # of the line still records the north star's denominator)
                out["cpu_baseline"]["same_reference_on_this_gpu_rays_per_s"] = g["value"]
                out["cpu_baseline"]["same_reference_on_this_gpu_ms_per_step"] = g["ms_per_step"]
        if world == 1 and H == 32 and not args.no_frame:
            # a REAL frame (objects + background model): driver-visible, untimed in `value`; a failure here cannot lose the line
            try:
                out["frame"] = frame_leg(cfg, dev, ipf, fargs)
            except Exception as e:
                out["frame"] = {"error": f"{type(e).__name__}: {e}"}
        if world == 1 and args.config == "replica_room0_vmap" and args.kernel == "auto" and not args.no_other_configs:
            # the other BASELINE configurations and the background step, measured like `value` (driver-visible; never part of it)
            legs = (("configs[0]", "imap_plumbing", "f32", False),
                    # the config-faithful iMAP batch (configs/Replica/config_replica_room0_iMAP.json: n_per_optim 4800, 9 + 5 bins, hidden 256)
                    ("configs[0]_as_the_reference_config_4800_rays", "imap_full", "f32", False),
                    ("configs[3]", "scannet0024_vmap", "bf16", False),
                    ("configs[3]_f32_weights", "scannet0024_vmap", "f32", False),
                    ("configs[4]_per_gpu_share", "stress_rank8", "bf16", False), ("configs[4]_on_one_gpu", "stress_256x64", "bf16", False),
                    ("background_step", "background", "f32", False),
                    ("configs[1]_ray_handoff", "replica_room0_vmap", "f32", True), ("background_step_ray_handoff", "background", "f32", True))
            oc = {}
            for label, cname, wts, as_rays in legs:
                try:
                    oc[label] = other_config_leg(cname, wts, dev, ipf, rays=as_rays)
                except Exception as e:
                    oc[label] = {"error": f"{type(e).__name__}: {e}"}
            out["other_configs"] = oc
        if world == 1 and args.config == "replica_room0_vmap" and args.kernel == "auto" and args.weights == "f32" and not args.no_precision:
            try:
                out["precision"] = precision_leg(dev)
            except Exception as e:
                out["precision"] = {"error": f"{type(e).__name__}: {e}"}
    # ---- the shared background model next to the objects (N > 1, or --with-background): AFTER everything the scored line needs,
    #      under a watchdog - this path (RCCL on a side stream, one communicator shared with the objects' flag reduction) has
    #      never run on an 8-GPU node, and a hang or an exception in it must not take `value` with it ----
    if (args.with_background or (world > 1 and args.full)) and not args.no_background:
        def on_timeout():
            if rank == 0:
                out["with_background"] = {"error": f"watchdog: the background legs did not finish within {args.bg_timeout:.0f} s (objects-only `value` above is unaffected)"}
                emit(out)
            os._exit(0)
        dog = Watchdog(args.bg_timeout, on_timeout)
        try:
            res = background_legs(args, cfg, dev, rank, world, ipf, dist, run_objects=lambda k: (bound.train_steps(k) if bound is not None else
                                  op.train_steps(tfc, tB, tsc, *fargs, opt=opt, n_steps=k, flag_reduce=flag_reduce)), rays_per_step=rays_per_step)
            if rank == 0:
                out["with_background"] = res
        except Exception as e:                       # reported, never fatal
            if rank == 0:
                out["with_background"] = {"error": f"{type(e).__name__}: {e}"}
        dog.cancel()
    if dist:
        # leaving together matters less than leaving: a rank whose background leg failed must not hang the others here
        dog = Watchdog(60.0, lambda: (emit(out) if rank == 0 else None, os._exit(0)))
        td.barrier()
        td.destroy_process_group()       # (RCCL prints its version banner on stdout: the JSON line comes after it, last)
        dog.cancel()
    if rank == 0 and world == 1 and args.full and not args.pmc_file and not args.no_pmc:
        # HBM-side bytes per launch, OBSERVED for the library this process runs: two rocprofv3 --pmc subprocess passes.  LAST, and under
        # a watchdog: a slow or hung profiler can cost the observation (the line then keeps the committed counter file's figure and
        # says so), never the line
        dog = Watchdog(2.0 * args.pmc_timeout + 20.0, lambda: (emit(out), os._exit(0)))
        try:
            t_obs, note = observe_traffic(args.config, args.weights, timeout_s=args.pmc_timeout)
            if t_obs is not None:
                out["roofline"]["traffic"] = t_obs
                out["roofline"]["traffic_source"] = note
            else:
                out["roofline"]["traffic_source"] = "could not observe (" + str(note) + "); " + str(out["roofline"].get("traffic_source"))
        except Exception as e:
            out["roofline"]["traffic_source"] = f"could not observe ({type(e).__name__}: {e}); " + str(out["roofline"].get("traffic_source"))
        dog.cancel()
    if rank == 0:
        emit(out)


if __name__ == "__main__":
    main()
