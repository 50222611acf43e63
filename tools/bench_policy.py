#!/usr/bin/env python3
"""Time the closed-loop policy's device side against the reference's host recipe.  JSON lines, appended to
profiles/policy_bench.jsonl; needs the GPU.

The reference's defaults: obs_horizon 10, step_size 5 (a history of L = 50 observations per environment), uint8 frames.

measure "policy_kernels", one line per E in --envs (default 1,64,1024).  Device events around --calls back-to-back calls (one
  call of a microsecond kernel would time the event pair), arms alternating in one process, median of --iters after a warm-up;
  the figures are microseconds PER CALL and include the host's enqueue where that is the longer.
  observe_us:      ClosedLoopPolicy.observe from device inputs, steady state (ONE spdm_policy_push launch);
  observe_fill_us: the same with every environment pending a fill (the observation goes into all L slots);
  batch_us:        ClosedLoopPolicy.batch (ONE spdm_policy_window launch, five torch.empty);
  unnormalize_us:  ClosedLoopPolicy.unnormalize (ONE spdm_policy_unnormalize launch, two torch.empty);
  *_copy_us:       a plain device copy (Tensor.clone) moving the same bytes -- half of (bytes read + bytes written) cloned:
                   what the memory system alone takes for that traffic;
  *_gbps:          (bytes read + bytes written) over the time;
  host_ms:         the reference's recipe on the host, wall clock, run once per environment: four deque appends,
                   torch.tensor(list(deque)[::s], dtype=float32) over the frames and the low-dimensional values, / 255,
                   permute, normalize_data / normalize_position on the CPU, and .to(device) of the five tensors
                   (run_predictions.py:30-60, :145-149), ending in a device synchronise.  For E > 16 the recipe is timed on 16
                   environments and scaled to E (host_envs_timed says how many ran): it is a loop over independent environments.
measure "control_period", E = 1: one control period with --steps-step DDIM (default 100) on UNet_Film, obs 10 / pred 22 /
  inpaint 10 (H = 32), D = 5, wall clock around a synchronised period, arms alternating.
  device_ms: observe (host inputs, as an environment hands them over) + plan;
  host_ms:   the host recipe above + model.sample + .cpu() + numpy unnormalize_position (run_predictions.py:145-164).

usage: python tools/bench_policy.py [--envs 1,64,1024] [--steps S] [--iters N] [--calls K] [--no-append]"""
import json
import os
import statistics
import sys
import time
import types
import warnings
from collections import deque

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from state_policy_diffusionmodel_amd.diffusion import load_model
from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
from state_policy_diffusionmodel_amd.weights import normalize_data, normalize_position, unnormalize_position

OBS, STEP, PRED, INP, D = 10, 5, 22, 10, 5
L = OBS * STEP
HOST_ENVS = 16
FRAME = 96 * 96 * 3
OUT = os.path.join(ROOT, "profiles", "policy_bench.jsonl")
STATS = {"position": {"min": np.float64(-37.3), "max": np.float64(52.9)},
         "velocity": {"min": np.array([-40.0, -38.0]), "max": np.array([41.0, 39.0])},
         "action": {"min": np.array([-1.0, 0.0, 0.0]), "max": np.array([1.0, 0.95, 0.8])}}


# ---- the reference's host recipe ------------------------------------------------------------------------------------------------
class HostLoop:
    """The four deques of one environment, filled as run_predictions.py:112-124 fills them."""

    def __init__(self, obs):
        self.bufs = [deque(maxlen=L) for _ in range(4)]
        for buf, x in zip(self.bufs, obs):
            for _ in range(L):
                buf.append(x)

    def step(self, obs, device):
        for buf, x in zip(self.bufs, obs):
            buf.append(x)
        with warnings.catch_warnings():                                         # torch warns that a list of arrays is slow: it is the recipe
            warnings.simplefilter("ignore", UserWarning)
            img, pos, vel, act = (torch.tensor(list(buf)[::STEP], dtype=torch.float32) for buf in self.bufs)
        npos, tr = normalize_position(pos, STATS["position"])
        batch = {"image": (img / 255.0).permute(0, 3, 1, 2).unsqueeze(0), "position": npos.unsqueeze(0),
                 "velocity": normalize_data(vel, STATS["velocity"]).float().unsqueeze(0),      # .float(): models/diffusion_ddpm.py:287-290
                 "action": normalize_data(act, STATS["action"]).float().unsqueeze(0),
                 "translation": tr.unsqueeze(0)}
        return {k: v.to(device) for k, v in batch.items()}


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
    rng = np.random.default_rng(E)
    host_obs = _observation(rng, E)
    obs = tuple(torch.from_numpy(x).to(dev) for x in host_obs)
    obs = (obs[0],) + tuple(x.float() for x in obs[1:])
    for _ in range(L + 3):
        policy.observe(*obs)
    x_0 = torch.rand(E, 1, PRED + INP, D, device=dev)
    tr = policy.batch()["translation"]

    def observe_fill():
        policy.reset()
        policy.observe(*obs)

    push_bytes = 2 * E * (FRAME + 28)                                           # read + write: a uint8 frame and 7 floats
    fill_bytes = E * (FRAME + 28) * (1 + L)
    window_bytes = E * OBS * (FRAME + 28) + E * OBS * (4 * FRAME + 28) + 8 * E
    unnorm_bytes = E * PRED * (4 * D + 8 * 5) + 8 * E
    clones = {k: torch.empty(max(n // 2, 16), dtype=torch.uint8, device=dev) for k, n in
              (("observe", push_bytes), ("observe_fill", fill_bytes), ("batch", window_bytes), ("unnormalize", unnorm_bytes))}
    arms = {"observe_us": lambda: policy.observe(*obs), "observe_copy_us": clones["observe"].clone,
            "observe_fill_us": observe_fill, "observe_fill_copy_us": clones["observe_fill"].clone,
            "batch_us": policy.batch, "batch_copy_us": clones["batch"].clone,
            "unnormalize_us": lambda: policy.unnormalize(x_0, tr), "unnormalize_copy_us": clones["unnormalize"].clone}
    us = {k: [] for k in arms}
    for it in range(iters + 2):
        for k, fn in arms.items():
            t = _device_us(fn, calls)
            if it >= 2:
                us[k].append(t)
    # the host recipe, once per environment; beyond HOST_ENVS environments that many are timed and the figure is scaled to E
    loop = HostLoop(tuple(x[0] for x in host_obs))
    timed = min(E, HOST_ENVS)
    host_ms = []
    for it in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for e in range(timed):
            batch = loop.step(tuple(x[e] for x in host_obs), dev)
        torch.cuda.synchronize()
        if it >= 1:
            host_ms.append((time.perf_counter() - t0) * 1e3 * E / timed)
        del batch
    res = {"measure": "policy_kernels", "E": E, "obs_h": OBS, "step_size": STEP, "L": L, "image_storage": "uint8", "iters": iters,
           "calls": calls, "ring_mib": round(E * L * FRAME / 2 ** 20, 1)}
    for k, v in us.items():
        res[k] = round(statistics.median(v), 2)
    for k, n in (("observe", push_bytes), ("observe_fill", fill_bytes), ("batch", window_bytes), ("unnormalize", unnorm_bytes)):
        res[k + "_bytes"] = n
        res[k + "_gbps"] = round(n / (res[k + "_us"] * 1e-6) / 1e9, 1)
        res[k + "_over_copy"] = round(res[k + "_us"] / res[k + "_copy_us"], 3)
    res["host_ms"], res["host_envs_timed"] = round(statistics.median(host_ms), 2), timed
    res["host_over_device"] = round(res["host_ms"] * 1e3 / (res["observe_us"] + res["batch_us"]), 1)
    return res


def control_period(steps, iters):
    from oracle.encoder_ref import make_encoder_state_dict
    model = load_model("DDIM", None, None, num_of_ddim_steps=steps, model="UNet_Film", noise_steps=steps, obs_horizon=OBS, pred_horizon=PRED,
                       inpaint_horizon=INP, observation_dim=135, prediction_dim=D, step_size=STEP,
                       vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=1)
    dev = model.device
    policy = ClosedLoopPolicy(model, STATS, n_envs=1, image_storage="uint8")
    rng = np.random.default_rng(1)
    stream = [_observation(rng, 1) for _ in range(8)]
    loop = HostLoop(tuple(x[0] for x in stream[0]))
    policy.observe(*stream[0])
    x_T = torch.rand(1, 1, PRED + INP, D, device=dev)
    pos_stats = STATS["position"]

    def device_arm(obs):
        policy.observe(*obs)
        return policy.plan(seed=0, x_T=x_T).waypoints

    def host_arm(obs):
        batch = loop.step(tuple(x[0] for x in obs), dev)
        translation = batch["translation"][0]
        pred = model.sample(batch, seed=0, x_T=x_T)[0, 0, INP:, :2].cpu().numpy()
        return unnormalize_position(pred, translation.cpu().numpy(), pos_stats)

    arms = {"device_ms": device_arm, "host_ms": host_arm}
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
    res = {"measure": "control_period", "E": 1, "obs_h": OBS, "step_size": STEP, "H": PRED + INP, "D": D, "model": "UNet_Film",
           "ddim_steps": steps, "iters": iters, "graph_captures_after_warmup": captures, "graph_captures_at_end": model._engine.graph_captures}
    for k, v in ms.items():
        res[k], res[k.replace("_ms", "_min_ms")] = round(statistics.median(v), 3), round(min(v), 3)
    res["host_minus_device_ms"] = round(res["host_ms"] - res["device_ms"], 3)
    return res


def main():
    args = sys.argv[1:]
    opts = {"--envs": "1,64,1024", "--steps": "100", "--iters": "7", "--calls": "20"}
    for flag in opts:
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    append = "--no-append" not in args
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy needs the GPU: there is nothing to time without it")
    envs, steps, iters, calls = [int(e) for e in opts["--envs"].split(",")], int(opts["--steps"]), int(opts["--iters"]), int(opts["--calls"])
    for fn in [lambda E=E: kernel_timing(E, iters, calls) for E in envs] + [lambda: control_period(steps, iters)]:
        line = json.dumps(fn())
        print(line, flush=True)
        if append:
            with open(OUT, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
