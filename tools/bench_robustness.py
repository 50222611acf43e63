#!/usr/bin/env python3
"""Time the observation noise and evaluation.robustness.  JSON lines, appended to
profiles/obs_noise_bench.jsonl; needs the GPU.

measure "obs_noise": the perturbation alone, device events, arms alternating in one process, median of --iters after a warm-up.
  hip:   noising.perturb_observations -- ONE spdm_obs_noise launch over the frames, positions, velocities and actions of 4096
         windows (obs 2 of 33 rows): cut and perturbed, 8 bytes of traffic per element;
  torch: the reference's recipe with torch-ROCm, per tensor  src[:, :obs] + alpha * torch.rand_like(src[:, :obs])
         (evaluation/eval_robustness.py:180-190; a rand kernel, a scale and an add where torch does not fuse them);
  copy:  the same cut with no noise, per tensor  src[:, :obs].clone()  -- the same 8 bytes per element and no arithmetic: what
         the memory system alone takes.  hip close to copy means the kernel is bound by HBM, well above it by the Philox rounds.
  "gbps" is 8 bytes x elements over the hip time, "peak_share" that over the 8 TB/s HBM peak.
measure "robustness": a whole evaluation.robustness call over 10 levels against ten host-style passes, host clock around a
  synchronised call: per level gather, torch.rand_like on the four tensors, sample, .cpu(), tests/eval_ref.py, numpy statistics.
  4096 windows x 1 run, batch_size 4096, obs 2 / pred 31 / inpaint 1 (H = 32), D = 5, UNet_Film, --steps-step DDIM (default 20).

usage: python tools/bench_robustness.py [--steps S] [--iters N] [--no-append]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import eval_ref
from state_policy_diffusionmodel_amd import evaluation
from state_policy_diffusionmodel_amd.dataset import DeviceDataset
from state_policy_diffusionmodel_amd.diffusion import load_model
from state_policy_diffusionmodel_amd.noising import OBSERVATION_KEYS, perturb_observations

OBS, PRED, INP, D, WINDOWS, BATCH, EPISODE, SEED = 2, 31, 1, 5, 4096, 4096, 1000, 0
LEVELS = evaluation.DEFAULT_LEVELS
HBM_PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "obs_noise_bench.jsonl")


def torch_perturb(batch, alpha):
    out = {}
    for k in OBSERVATION_KEYS:
        src = batch[k][:, :OBS]
        out[k] = src + alpha * torch.rand_like(src)
    return out


def kernel_timing(ds, iters):
    batch = ds.batch(np.arange(WINDOWS), frames="obs")
    arms = {"hip_us": lambda: perturb_observations(batch, 0.05, obs_horizon=OBS, seed=SEED, draw=1, row_offset=0),
            "torch_us": lambda: torch_perturb(batch, 0.05),
            "copy_us": lambda: {k: batch[k][:, :OBS].clone() for k in OBSERVATION_KEYS}}
    us = {k: [] for k in arms}
    for it in range(iters + 2):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            del out
            if it >= 2:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    elements = sum(batch[k][:, :OBS].numel() for k in OBSERVATION_KEYS)
    res = {"measure": "obs_noise", "windows": WINDOWS, "obs_h": OBS, "elements": elements, "frame_elements": batch["image"].numel(),
           "iters": iters}
    for k, v in us.items():
        res[k], res[k.replace("_us", "_min_us")] = round(statistics.median(v), 1), round(min(v), 1)
    res["torch_over_hip"] = round(res["torch_us"] / res["hip_us"], 3)
    res["hip_over_copy"] = round(res["hip_us"] / res["copy_us"], 3)
    res["gbps"] = round(8.0 * elements / (res["hip_us"] * 1e-6) / 1e9, 1)
    res["peak_share"] = round(8.0 * elements / (res["hip_us"] * 1e-6) / HBM_PEAK, 3)
    return res


def host_way(model, ds, ids, x_T):
    """Ten separate passes the way a user would write them today; the statistics of evaluation.robustness in numpy."""
    st, out = ds.stats, []
    for alpha in LEVELS:
        pos, act = [], []
        for g0, g1, k0, k1 in evaluation.chunks(len(ids), 1, BATCH):
            batch = ds.batch(ids[k0:k1], frames="obs", with_translation=True)
            obs = model.prepare_observation_batch(torch_perturb(batch, alpha) if alpha else batch)
            cond, inpaint = model.prepare_obs_cond_vectors(obs), model.prepare_inpaint_vectors(obs)
            x_0 = model.sample({"obs_cond": cond, "inpaint": inpaint}, batched=True, sharded=False, x_T=x_T[g0:g1], seed=SEED,
                               sample_offset=g0).cpu().numpy()[:, 0]
            slot = eval_ref.slots(g0, g1 - g0, 1, k0)
            tp, ta, tr = (batch[k].cpu().numpy() for k in ("position", "action", "translation"))
            pos.append(eval_ref.position_errors(x_0, tp, tr, slot, float(st["position"]["min"]), float(st["position"]["max"]), OBS, INP, PRED))
            act.append(eval_ref.action_errors(x_0, ta, slot, st["action"]["min"], st["action"]["max"], OBS, INP, PRED))
        pos, act = np.concatenate(pos), np.concatenate(act)
        out.append({"position_error": pos, "mean_error": pos.mean(axis=0), "std_error": pos.std(axis=0), "action_mean_error": act.mean(axis=0),
                    "action_std_error": act.std(axis=0), "mse_position": np.mean(np.square(pos)) / 2, "mse_action": np.mean(np.square(act))})
    return out


def evaluation_timing(ds, steps, iters):
    from oracle.encoder_ref import make_encoder_state_dict
    model = load_model("DDIM", None, None, num_of_ddim_steps=steps, model="UNet_Film", noise_steps=steps, obs_horizon=OBS, pred_horizon=PRED,
                       inpaint_horizon=INP, observation_dim=135, prediction_dim=D, vision_encoder_state_dict=make_encoder_state_dict(7),
                       max_batch=BATCH)
    ids = np.arange(WINDOWS, dtype=np.int64)
    x_T = evaluation.initial_noise(model, WINDOWS, SEED)
    arms = {"device_ms": lambda: evaluation.robustness(model, ds, ids, levels=LEVELS, runs=1, batch_size=BATCH, seed=SEED),
            "host_ms": lambda: host_way(model, ds, ids, x_T)}
    rep, ref = arms["device_ms"](), arms["host_ms"]()                  # warm-up; level 0 has no noise, so there the two arms agree
    same = bool(np.array_equal(rep.position_error[0].reshape(ref[0]["position_error"].shape), ref[0]["position_error"]))
    ms = {k: [] for k in arms}
    for _ in range(iters):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {"measure": "robustness", "windows": WINDOWS, "runs": 1, "levels": len(LEVELS), "batch_size": BATCH, "H": PRED + INP, "D": D,
           "ddim_steps": steps, "iters": iters, "level0_bit_equal": same,
           "mse_position": [float(f"{v:.6g}") for v in rep.mse_position], "mse_action": [float(f"{v:.6g}") for v in rep.mse_action]}
    for k, v in ms.items():
        res[k], res[k.replace("_ms", "_min_ms")] = round(statistics.median(v), 2), round(min(v), 2)
    res["host_over_device"] = round(res["host_ms"] / res["device_ms"], 3)
    return res


def main():
    args = sys.argv[1:]
    steps, iters = 20, 5
    for flag in ("--steps", "--iters"):
        if flag in args:
            i = args.index(flag)
            val = int(args[i + 1])
            del args[i:i + 2]
            steps, iters = (val, iters) if flag == "--steps" else (steps, val)
    append = "--no-append" not in args
    if not torch.cuda.is_available():
        raise SystemExit("bench_robustness needs the GPU: there is nothing to time without it")
    T = EPISODE * (-(-WINDOWS // (EPISODE - OBS - PRED + 1)))
    rng = np.random.default_rng(0)
    ds = DeviceDataset(30.0 * rng.standard_normal((T, 2)), rng.standard_normal((T, 2)), rng.uniform(-1, 1, (T, 3)),
                       rng.integers(0, 256, (T, 96, 96, 3), dtype=np.uint8), np.arange(EPISODE, T + 1, EPISODE), PRED, OBS, step_size=1)
    for res in (kernel_timing(ds, iters), evaluation_timing(ds, steps, iters)):
        line = json.dumps(res)
        print(line, flush=True)
        if append:
            with open(OUT, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
