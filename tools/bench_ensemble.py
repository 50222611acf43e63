#!/usr/bin/env python3
"""Time planning from K candidates per environment.  JSON lines, appended to profiles/ensemble_bench.jsonl (or
--out); needs the GPU.  The discipline is tools/bench_policy.py's: one process, arms alternating, median of --iters after a
warm-up.

The reference's geometry: obs_horizon 10, step_size 5, pred_horizon 22, inpaint_horizon 10 (H = 32), D = 5.

measure "select_kernel", one line per E in --envs (default 1,4,16,64,256,1024) at K = --k (default 16), and one at E = 1, K = 64.
  Device events around --calls back-to-back calls; microseconds PER CALL, which include the host's enqueue where that is the
  longer.  ClosedLoopPolicy.select: ONE spdm_policy_select launch and four torch.empty.
  medoid_us, coherent_us: cols = 2 (positions), scores and spread written;  medoid5_us: cols = 5 (positions and actions);
  warm_start_us: ClosedLoopPolicy.warm_start over the same E environments, the enqueue floor the launch is held against.
measure "ensemble_control_period", E = 1, UNet_Film, one line per schedule: --steps-step DDIM (default 100) and DPM-Solver++ (2M)
  with --solver steps (default 10).  Wall clock around a synchronised observe + plan_candidates(candidates=K), K in
  --candidates (default 1,4,16,64), all on one policy; select = 'coherent', so every timed plan makes the guess launch and the select launch.
  k<K>_ms: the periods (k1_ms: plan()'s calls);  k<K>_over_k1: their ratio to the K = 1 period of the same round, median.

usage: python tools/bench_ensemble.py [--envs 1,4,...] [--k K] [--steps N] [--solver N] [--candidates 1,4,16,64] [--iters N]
                                      [--calls K] [--out PATH]"""
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from state_policy_diffusionmodel_amd.diffusion import load_model
from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy

OBS, STEP, PRED, INP, D = 10, 5, 22, 10, 5
H = PRED + INP
OUT = os.path.join(ROOT, "profiles", "ensemble_bench.jsonl")
STATS = {"position": {"min": np.float64(-37.3), "max": np.float64(52.9)},
         "velocity": {"min": np.array([-40.0, -38.0]), "max": np.array([41.0, 39.0])},
         "action": {"min": np.array([-1.0, 0.0, 0.0]), "max": np.array([1.0, 0.95, 0.8])}}


def _observation(rng, E):
    return (rng.integers(0, 256, (E, 96, 96, 3), dtype=np.uint8), 30.0 * rng.standard_normal((E, 2)),
            12.0 * rng.standard_normal((E, 2)), rng.uniform(-1.0, 1.0, (E, 3)))


def _device_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1) * 1e3 / calls


def kernel_timing(E, K, iters, calls):
    dev = torch.device("cuda", 0)
    geometry = types.SimpleNamespace(obs_horizon=OBS, pred_horizon=PRED, inpaint_horizon=INP, prediction_dim=D, step_size=STEP, device=dev)
    policy = ClosedLoopPolicy(geometry, STATS, n_envs=E, image_storage="uint8")
    gen = torch.Generator(device=dev).manual_seed(E * 100 + K)
    x = torch.rand(E * K, 1, H, D, device=dev, generator=gen) * 2 - 1
    guess = torch.rand(E, H, D, device=dev, generator=gen) * 2 - 1
    T0 = torch.rand(E, 2, device=dev, generator=gen) * 2 - 1
    inpaint = torch.rand(E, INP, D, device=dev, generator=gen) * 2 - 1
    arms = {"medoid_us": lambda: policy.select(x, K, "medoid", cols=2, translation=T0),
            "coherent_us": lambda: policy.select(x, K, "coherent", guess=guess, rows=PRED - 10, cols=2, translation=T0),
            "medoid5_us": lambda: policy.select(x, K, "medoid", cols=D, translation=T0),
            "warm_start_us": lambda: policy.warm_start(guess, T0, T0, inpaint, 50, 0.83, 0.56, 11, 3)}
    us = {k: [] for k in arms}
    for it in range(iters + 2):
        for k, fn in arms.items():
            t = _device_us(fn, calls)
            if it >= 2:
                us[k].append(t)
    res = {"measure": "select_kernel", "E": E, "K": K, "H": H, "D": D, "inp_h": INP, "rows": PRED - 10, "iters": iters, "calls": calls}
    for k, v in us.items():
        res[k] = round(statistics.median(v), 2)
    return res


def control_period(schedule, steps, candidates, iters):
    from oracle.encoder_ref import make_encoder_state_dict
    common = dict(model="UNet_Film", obs_horizon=OBS, pred_horizon=PRED, inpaint_horizon=INP, observation_dim=135, prediction_dim=D,
                  step_size=STEP, vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=max(candidates))
    if schedule == "ddim":
        model = load_model("DDIM", None, None, num_of_ddim_steps=steps, noise_steps=steps, **common)
    else:
        model = load_model("DDPM", None, None, noise_steps=1000, solver_steps=steps, **common)
    dev = model.device
    policy = ClosedLoopPolicy(model, STATS, n_envs=1, image_storage="uint8")
    rng = np.random.default_rng(1)
    stream = [_observation(rng, 1) for _ in range(8)]
    policy.observe(*stream[0])
    x_T = {K: torch.rand(K, 1, H, D, device=dev) for K in candidates}
    policy.plan(seed=0, x_T=x_T[1] if 1 in x_T else None)                   # the plan the first coherent selection refers to

    def period(K):
        def arm(obs):
            policy.observe(*obs)
            plan = policy.plan_candidates(seed=0, x_T=x_T[K], candidates=K)
            assert plan.candidates == K and plan.selected_by == ("coherent" if K > 1 else ""), (K, plan.selected_by)
        return arm

    arms = {f"k{K}_ms": period(K) for K in candidates}
    ms = {k: [] for k in arms}
    for it in range(iters + 2):
        obs = stream[it % len(stream)]
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(obs)
            torch.cuda.synchronize()
            if it >= 2:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {"measure": "ensemble_control_period", "E": 1, "obs_h": OBS, "step_size": STEP, "H": H, "D": D, "model": "UNet_Film",
           "schedule": schedule, "steps": steps, "iters": iters, "select": "coherent", "cols": 2}
    for k, v in ms.items():
        res[k], res[k.replace("_ms", "_min_ms")] = round(statistics.median(v), 3), round(min(v), 3)
    if "k1_ms" in ms:
        for K in candidates:
            if K > 1:
                res[f"k{K}_over_k1"] = round(statistics.median(a / b for a, b in zip(ms[f"k{K}_ms"], ms["k1_ms"])), 4)
    return res


def main():
    args = sys.argv[1:]
    opts = {"--envs": "1,4,16,64,256,1024", "--k": "16", "--steps": "100", "--solver": "10", "--candidates": "1,4,16,64", "--iters": "7",
            "--calls": "20", "--out": OUT}
    for flag in opts:
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble needs the GPU: there is nothing to time without it")
    envs, K, iters, calls = [int(e) for e in opts["--envs"].split(",")], int(opts["--k"]), int(opts["--iters"]), int(opts["--calls"])
    candidates = [int(k) for k in opts["--candidates"].split(",")]
    lines = [kernel_timing(E, K, iters, calls) for E in envs] + [kernel_timing(1, 64, iters, calls)]
    lines.append(control_period("ddim", int(opts["--steps"]), candidates, iters))
    lines.append(control_period("dpmsolver++2m", int(opts["--solver"]), candidates, iters))
    for res in lines:
        line = json.dumps(res)
        print(line, flush=True)
        with open(opts["--out"], "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
