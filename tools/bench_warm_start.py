#!/usr/bin/env python3
"""Time warm-started replanning.  JSON lines, appended to profiles/warm_start_bench.jsonl (or --out); needs the
GPU.  The discipline is tools/bench_policy.py's: one process, arms alternating, median of --iters after a warm-up.

The reference's geometry: obs_horizon 10, step_size 5, pred_horizon 22, inpaint_horizon 10 (H = 32), D = 5.

measure "warm_start_kernel", one line per E in --envs (default 1,64,1024).  Device events around --calls back-to-back calls;
  microseconds PER CALL, which include the host's enqueue where that is the longer.
  warm_start_us: ClosedLoopPolicy.warm_start (ONE spdm_policy_warm_start launch, one torch.empty), noise drawn;
  copy_us:       a plain device copy (Tensor.clone) moving the same bytes -- half of (bytes read + bytes written) cloned;
  gbps:          (bytes read + bytes written) over warm_start_us.
measure "warm_control_period", E = 1: --steps-step DDIM (default 100) on UNet_Film, wall clock around a synchronised
  observe + plan, for a cold plan and for plan(warm_start=K), K in --warm (default 10,20,50).
  cold_ms, warm<K>_ms: the periods;  sample_ms: model.sample alone on the cold plan's batch (all N steps);
  outside_ms = cold_ms - sample_ms: what a period spends outside sample();
  predicted<K>_ms = sample_ms K / N + outside_ms + the warm-start launch (warm_start_us of E = 1, measured in this process);
  residual<K>_ms = warm<K>_ms - predicted<K>_ms.

usage: python tools/bench_warm_start.py [--envs 1,64,1024] [--steps N] [--warm 10,20,50] [--iters N] [--calls K] [--out PATH]"""
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
OUT = os.path.join(ROOT, "profiles", "warm_start_bench.jsonl")
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


def kernel_timing(E, iters, calls):
    dev = torch.device("cuda", 0)
    geometry = types.SimpleNamespace(obs_horizon=OBS, pred_horizon=PRED, inpaint_horizon=INP, prediction_dim=D, step_size=STEP, device=dev)
    policy = ClosedLoopPolicy(geometry, STATS, n_envs=E, image_storage="uint8")
    gen = torch.Generator(device=dev).manual_seed(E)
    prev = torch.rand(E, 1, H, D, device=dev, generator=gen) * 2 - 1
    T0 = torch.rand(E, 2, device=dev, generator=gen) * 2 - 1
    T1 = T0 + 0.01
    inpaint = torch.rand(E, INP, D, device=dev, generator=gen) * 2 - 1
    nbytes = E * (2 * H * D * 4 + INP * D * 4 + 16)                         # read: plan, in-paint rows, two translations; write: x
    clone = torch.empty(max(nbytes // 2, 16), dtype=torch.uint8, device=dev)
    arms = {"warm_start_us": lambda: policy.warm_start(prev, T0, T1, inpaint, 50, 0.83, 0.56, 11, 3), "copy_us": clone.clone}
    us = {k: [] for k in arms}
    for it in range(iters + 2):
        for k, fn in arms.items():
            t = _device_us(fn, calls)
            if it >= 2:
                us[k].append(t)
    res = {"measure": "warm_start_kernel", "E": E, "H": H, "D": D, "inp_h": INP, "step_size": STEP, "delta": 50, "iters": iters,
           "calls": calls, "bytes": nbytes}
    for k, v in us.items():
        res[k] = round(statistics.median(v), 2)
    res["gbps"] = round(nbytes / (res["warm_start_us"] * 1e-6) / 1e9, 2)
    res["over_copy"] = round(res["warm_start_us"] / res["copy_us"], 3)
    return res


def control_period(steps, warm, iters, launch_us):
    from oracle.encoder_ref import make_encoder_state_dict
    model = load_model("DDIM", None, None, num_of_ddim_steps=steps, model="UNet_Film", noise_steps=steps, obs_horizon=OBS, pred_horizon=PRED,
                       inpaint_horizon=INP, observation_dim=135, prediction_dim=D, step_size=STEP,
                       vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=1)
    dev = model.device
    policy = ClosedLoopPolicy(model, STATS, n_envs=1, image_storage="uint8")
    rng = np.random.default_rng(1)
    stream = [_observation(rng, 1) for _ in range(8)]
    policy.observe(*stream[0])
    x_T = torch.rand(1, 1, H, D, device=dev)
    state = {}

    def period(K):
        def arm(obs):
            policy.observe(*obs)
            plan = policy.plan(seed=0, x_T=x_T, warm_start=K)
            assert plan.warm is (K is not None) and plan.steps == (K or steps), (K, plan.warm, plan.steps)
        return arm

    def sample_arm(obs):
        model.sample(dict(state["cond"]), batched=True, sharded=False, seed=0, x_T=x_T)

    policy.plan(seed=0, x_T=x_T)                                            # the plan the first warm arm starts from
    state["cond"] = policy.batch()
    arms = {"cold_ms": period(None), "sample_ms": sample_arm}
    arms.update({f"warm{K}_ms": period(K) for K in warm})
    ms = {k: [] for k in arms}
    captures = None
    for it in range(iters + 2):
        obs = stream[it % len(stream)]
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(obs)
            torch.cuda.synchronize()
            if it >= 2:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        if it == 1:
            captures = model._engine.graph_captures
    res = {"measure": "warm_control_period", "E": 1, "obs_h": OBS, "step_size": STEP, "H": H, "D": D, "model": "UNet_Film",
           "ddim_steps": steps, "iters": iters, "graph_captures_after_warmup": captures, "graph_captures_at_end": model._engine.graph_captures,
           "warm_start_launch_us": launch_us}
    for k, v in ms.items():
        res[k], res[k.replace("_ms", "_min_ms")] = round(statistics.median(v), 3), round(min(v), 3)
    res["outside_ms"] = round(res["cold_ms"] - res["sample_ms"], 3)
    for K in warm:
        predicted = res["sample_ms"] * K / steps + res["outside_ms"] + (launch_us or 0.0) * 1e-3
        res[f"predicted{K}_ms"] = round(predicted, 3)
        res[f"residual{K}_ms"] = round(res[f"warm{K}_ms"] - predicted, 3)
        res[f"warm{K}_over_cold"] = round(res[f"warm{K}_ms"] / res["cold_ms"], 4)
    return res


def main():
    args = sys.argv[1:]
    opts = {"--envs": "1,64,1024", "--steps": "100", "--warm": "10,20,50", "--iters": "7", "--calls": "20", "--out": OUT}
    for flag in opts:
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    if not torch.cuda.is_available():
        raise SystemExit("bench_warm_start needs the GPU: there is nothing to time without it")
    envs, steps, iters, calls = [int(e) for e in opts["--envs"].split(",")], int(opts["--steps"]), int(opts["--iters"]), int(opts["--calls"])
    warm = [int(k) for k in opts["--warm"].split(",")]
    lines = [kernel_timing(E, iters, calls) for E in envs]
    launch_us = next((r["warm_start_us"] for r in lines if r["E"] == 1), None)
    lines.append(control_period(steps, warm, iters, launch_us))
    for res in lines:
        line = json.dumps(res)
        print(line, flush=True)
        with open(opts["--out"], "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
