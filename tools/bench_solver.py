#!/usr/bin/env python3
"""Time and probe the DPM-Solver++ (2M) sampler against DDIM.  JSON lines, appended to profiles/solver_bench.jsonl;
needs the GPU.  Random-init weights throughout, as bench.py uses them.

measure "step_ms", one line per (route, B): a denoise step under SPDM_DPMPP_2M against one under SPDM_DDIM, H = 32, D = 3,
  cond 10 x 135, --steps-step loops (default 20) on a grid of 1000, two handles of one configuration timed alternately in one
  process, device events around spdm_sample_run(0, n) (graph replay), median of --iters after a warm-up, divided by n.
  route "film_attention": UNet_Film -- sa6's epilogue leaves eps, the solver's launch takes out_step's place: equal launch counts;
  route "no_attention":   UNet_FilmnoAttention -- out_step writes eps, the solver's launch follows: one small launch more.
measure "control_period", E = 1, cold plans: observe (host inputs) + plan, wall clock around a synchronised period, UNet_Film,
  obs 10 / pred 22 / inpaint 10 (H = 32), D = 5: the solver at n = 10 and n = 20 against DDIM-100, arms alternating.
measure "solver_error": B = 8 trajectories from one x_T on UNet_Film (H = 32, D = 3, exact fp32); the reference solution is DDIM
  at n = T = 1000; max |x_0(n) - x_0(ref)| for DDIM and for the solver with and without euler_at_final at n = 10, 20, 50.
  On an untrained network this measures how fast each scheme converges to ITS probability-flow solution, and says little about
  plan quality, which remains unmeasured.

usage: python tools/bench_solver.py [--batches 1,256,4096] [--steps S] [--iters N] [--only step_ms,control_period,solver_error] [--no-append]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from state_policy_diffusionmodel_amd.diffusion import load_model
from state_policy_diffusionmodel_amd.engine import SpdmEngine
from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
from state_policy_diffusionmodel_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
from state_policy_diffusionmodel_amd.weights import random_state_dict

OUT = os.path.join(ROOT, "profiles", "solver_bench.jsonl")
H, D, OBS_H, OBS_DIM, T = 32, 3, 10, 135, 1000
STATS = {"position": {"min": np.float64(-37.3), "max": np.float64(52.9)},
         "velocity": {"min": np.array([-40.0, -38.0]), "max": np.array([41.0, 39.0])},
         "action": {"min": np.array([-1.0, 0.0, 0.0]), "max": np.array([1.0, 0.95, 0.8])}}


def _scheduler(kind, n, **options):
    s = (DDIMScheduler if kind == "ddim" else DPMSolverMultistepScheduler)(num_train_timesteps=T, **options)
    s.set_timesteps(n)
    return s


def step_ms(attention, B, n, iters):
    sd = random_state_dict(OBS_H * OBS_DIM, seed=0, attention=attention)
    g = torch.Generator().manual_seed(B)
    cond = torch.randn(B, 1, OBS_H, OBS_DIM, generator=g).cuda()
    x_T = torch.rand(B, 1, H, D, generator=g).cuda()
    inpaint = (torch.rand(B, 1, 1, D, generator=g) * 2 - 1).cuda()
    engines = {}
    for kind in ("ddim", "dpmpp_2m"):
        eng = SpdmEngine(H, D, OBS_H * OBS_DIM, max_batch=B, attention=attention, num_train_timesteps=T)
        eng.load_state_dict(sd)
        eng.set_scheduler(_scheduler(kind, n))
        engines[kind] = eng
    ms = {k: [] for k in engines}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    try:
        for it in range(iters + 2):
            for kind, eng in engines.items():
                eng.sample_begin(cond, x_T, inpaint=inpaint)
                torch.cuda.synchronize()
                e0.record()
                eng.sample_run(0, n)
                e1.record()
                e1.synchronize()
                if it >= 2:
                    ms[kind].append(e0.elapsed_time(e1) / n)
        captures = {k: eng.graph_captures for k, eng in engines.items()}
    finally:
        for eng in engines.values():
            eng.close()
    res = {"measure": "step_ms", "route": "film_attention" if attention else "no_attention", "B": B, "H": H, "D": D, "steps": n,
           "iters": iters, "graph_captures": captures}
    for k, v in ms.items():
        res[k + "_ms"], res[k + "_min_ms"] = round(statistics.median(v), 4), round(min(v), 4)
    res["dpmpp_2m_over_ddim"] = round(res["dpmpp_2m_ms"] / res["ddim_ms"], 4)
    return res


def control_period(iters):
    from oracle.encoder_ref import make_encoder_state_dict
    obs_h, step, pred, inp, d = 10, 5, 22, 10, 5
    size = dict(model="UNet_Film", obs_horizon=obs_h, pred_horizon=pred, inpaint_horizon=inp, observation_dim=135, prediction_dim=d,
                step_size=step, vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=1)
    models = {"ddim_100": load_model("DDIM", None, None, num_of_ddim_steps=100, noise_steps=100, **size),
              "dpmpp_2m_10": load_model("DDPM", None, None, noise_steps=T, solver_steps=10, **size),
              "dpmpp_2m_20": load_model("DDPM", None, None, noise_steps=T, solver_steps=20, **size)}
    policies = {k: ClosedLoopPolicy(m, STATS, n_envs=1, image_storage="uint8") for k, m in models.items()}
    rng = np.random.default_rng(1)
    stream = [(rng.integers(0, 256, (1, 96, 96, 3), dtype=np.uint8), 30.0 * rng.standard_normal((1, 2)), 12.0 * rng.standard_normal((1, 2)),
               rng.uniform(-1.0, 1.0, (1, 3))) for _ in range(8)]
    x_T = torch.rand(1, 1, pred + inp, d, device="cuda")
    for p in policies.values():
        p.observe(*stream[0])
    ms = {k: [] for k in policies}
    for it in range(iters + 2):
        obs = stream[it % len(stream)]
        for k, p in policies.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.observe(*obs)
            p.plan(seed=0, x_T=x_T)
            torch.cuda.synchronize()
            if it >= 2:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {"measure": "control_period", "E": 1, "H": pred + inp, "D": d, "model": "UNet_Film", "iters": iters, "plans": "cold"}
    for k, v in ms.items():
        res[k + "_ms"], res[k + "_min_ms"] = round(statistics.median(v), 3), round(min(v), 3)
    return res


def solver_error():
    B = 8
    sd = random_state_dict(OBS_H * OBS_DIM, seed=0, attention=True)
    g = torch.Generator().manual_seed(7)
    cond = torch.randn(B, 1, OBS_H, OBS_DIM, generator=g).cuda()
    x_T = torch.rand(B, 1, H, D, generator=g).cuda()
    eng = SpdmEngine(H, D, OBS_H * OBS_DIM, max_batch=B, attention=True, num_train_timesteps=T, exact_fp32=True)
    eng.load_state_dict(sd)
    res = {"measure": "solver_error", "B": B, "H": H, "D": D, "model": "UNet_Film", "weights": "random init", "precision": "exact fp32",
           "reference": "DDIM n = T = 1000"}
    try:
        eng.set_scheduler(_scheduler("ddim", T))
        ref = eng.sample(cond, x_T)
        res["ref_max_abs"] = round(float(ref.abs().max()), 4)
        arms = (("ddim", "ddim", {}), ("dpmpp_2m", "solver", {}), ("dpmpp_2m_euler_at_final", "solver", {"euler_at_final": True}))
        for name, kind, options in arms:
            for n in (10, 20, 50):
                eng.set_scheduler(_scheduler(kind, n, **options))
                res[f"{name}_{n}"] = float(f"{float((eng.sample(cond, x_T) - ref).abs().max()):.4e}")
    finally:
        eng.close()
    return res


def main():
    args = sys.argv[1:]
    opts = {"--batches": "1,256,4096", "--steps": "20", "--iters": "7", "--only": "step_ms,control_period,solver_error"}
    for flag in opts:
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    append = "--no-append" not in args
    if not torch.cuda.is_available():
        raise SystemExit("bench_solver needs the GPU: there is nothing to time without it")
    batches, n, iters, only = [int(b) for b in opts["--batches"].split(",")], int(opts["--steps"]), int(opts["--iters"]), opts["--only"].split(",")
    jobs = []
    if "step_ms" in only:
        jobs += [lambda a=a, B=B: step_ms(a, B, n, iters) for a in (True, False) for B in batches]
    if "control_period" in only:
        jobs.append(lambda: control_period(iters))
    if "solver_error" in only:
        jobs.append(solver_error)
    for fn in jobs:
        line = json.dumps(fn())
        print(line, flush=True)
        if append:
            with open(OUT, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
