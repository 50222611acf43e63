#!/usr/bin/env python3
"""Time evaluation.evaluate.  One JSON line per size; needs the GPU.

Two arms over the SAME chunks, alternating in one process, host clock around a synchronised call:
  device: evaluate() -- per chunk one spdm_eval_errors launch behind the sampler, one spdm_eval_reduce and one read-back at the end;
  host:   per chunk sample -> .cpu() -> tests/eval_ref.py (numpy), then np.mean / np.std per window and over all rows.
K windows x 8 runs = 4096 and 16384 trajectories, batch_size 4096, obs 2 / pred 31 / inpaint 1 (H = 32), D = 5, UNet_Film under a
--steps-step DDIM schedule (default 20).  The sampler dominates both arms, so "metric_*" also times the metric alone with device
events on a resident x_0: errors_us = one spdm_eval_errors at B = 4096, reduce_us = spdm_eval_reduce over all rows (position
and action buffers).

usage: python tools/bench_eval.py [--steps S] [--iters N] [TRAJECTORIES ...]"""
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

OBS, PRED, INP, D, RUNS, BATCH, EPISODE, SEED = 2, 31, 1, 5, 8, 4096, 1000, 0


def host_way(model, ds, ids, x_T):
    N, st = len(ids) * RUNS, ds.stats
    pos, act = [], []
    for g0, g1, k0, k1 in evaluation.chunks(len(ids), RUNS, BATCH):
        batch = ds.batch(ids[k0:k1], frames="obs", with_translation=True)
        obs = model.prepare_observation_batch(batch)
        cond, inpaint = model.prepare_obs_cond_vectors(obs), model.prepare_inpaint_vectors(obs)
        slot = eval_ref.slots(g0, g1 - g0, RUNS, k0)
        sel = torch.from_numpy(slot).to(model.device)
        x_0 = model.sample({"obs_cond": cond[sel], "inpaint": inpaint[sel]}, batched=True, sharded=False, x_T=x_T[g0:g1], seed=SEED,
                           sample_offset=g0).cpu().numpy()[:, 0]
        tp, ta, tr = (batch[k].cpu().numpy() for k in ("position", "action", "translation"))
        pos.append(eval_ref.position_errors(x_0, tp, tr, slot, float(st["position"]["min"]), float(st["position"]["max"]), OBS, INP, PRED))
        act.append(eval_ref.action_errors(x_0, ta, slot, st["action"]["min"], st["action"]["max"], OBS, INP, PRED))
    pos, act = np.concatenate(pos), np.concatenate(act)
    out = {"position_error": pos, "action_error": act}
    for name, e in (("", pos), ("action_", act)):
        per = e.reshape((len(ids), RUNS) + e.shape[1:])
        out[name + "mean_error"], out[name + "std_error"] = e.mean(axis=0), e.std(axis=0)
        out[name + "window_mean"], out[name + "window_std"] = per.mean(axis=1), per.std(axis=1)
    assert pos.shape[0] == N
    return out


def metric_alone(model, ds, ids, iters):
    """Device-event times of the metric's launches on resident inputs."""
    k1 = BATCH // RUNS
    batch = ds.batch(ids[:k1], frames=None, with_translation=True)
    x_0 = torch.rand(BATCH, 1, PRED + INP, D, device=model.device)
    N = len(ids) * RUNS
    pos = torch.empty((N, PRED), dtype=torch.float64, device=model.device)
    act = torch.empty((N, PRED, 3), dtype=torch.float64, device=model.device)
    pos.uniform_(0, 1)
    act.uniform_(0, 1)

    def errors():
        evaluation.errors_into(x_0, batch, ds.stats, obs_h=OBS, inp_h=INP, runs=RUNS, first_traj=0, window_base=0, pos_err=pos[:BATCH],
                               act_err=act[:BATCH])

    def reduce():
        evaluation.reduce_errors(pos, RUNS)
        evaluation.reduce_errors(act.view(N, -1), RUNS)

    res = {}
    for name, fn in (("errors_us", errors), ("reduce_us", reduce)):
        us = []
        for it in range(iters + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 3:
                us.append(e0.elapsed_time(e1) * 1e3)
        res["metric_" + name] = round(statistics.median(us), 1)
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
    sizes = [int(a) for a in args] or [4096, 16384]
    if any(n < BATCH or n % RUNS for n in sizes):
        raise SystemExit(f"every size must be at least {BATCH} trajectories and a multiple of {RUNS} runs")
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval needs the GPU: there is nothing to time without it")
    from oracle.encoder_ref import make_encoder_state_dict
    K = max(sizes) // RUNS
    T = EPISODE * (-(-K // (EPISODE - OBS - PRED + 1)))
    rng = np.random.default_rng(0)
    ds = DeviceDataset(30.0 * rng.standard_normal((T, 2)), rng.standard_normal((T, 2)), rng.uniform(-1, 1, (T, 3)),
                       rng.integers(0, 256, (T, 96, 96, 3), dtype=np.uint8), np.arange(EPISODE, T + 1, EPISODE), PRED, OBS, step_size=1)
    model = load_model("DDIM", None, None, num_of_ddim_steps=steps, model="UNet_Film", noise_steps=steps, obs_horizon=OBS, pred_horizon=PRED,
                       inpaint_horizon=INP, observation_dim=135, prediction_dim=D, vision_encoder_state_dict=make_encoder_state_dict(7),
                       max_batch=BATCH)
    for n in sizes:
        ids = np.arange(n // RUNS, dtype=np.int64)
        x_T = evaluation.initial_noise(model, n, SEED)
        arms = {"device_ms": lambda: evaluation.evaluate(model, ds, ids, runs=RUNS, batch_size=BATCH, seed=SEED),
                "host_ms": lambda: host_way(model, ds, ids, x_T)}
        rep, ref = arms["device_ms"](), arms["host_ms"]()                  # warm-up, and the two arms agree before either is timed
        same = all(np.array_equal(getattr(rep, k), ref[k].reshape(getattr(rep, k).shape)) for k in ("position_error", "action_error"))
        ms = {k: [] for k in arms}
        for _ in range(iters):
            for k, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        out = {"measure": "evaluate", "trajectories": n, "windows": n // RUNS, "runs": RUNS, "batch_size": BATCH, "H": PRED + INP, "D": D,
               "ddim_steps": steps, "iters": iters, "errors_bit_equal": bool(same)}
        for k, v in ms.items():
            out[k], out[k.replace("_ms", "_min_ms")] = round(statistics.median(v), 2), round(min(v), 2)
        out["host_over_device"] = round(out["host_ms"] / out["device_ms"], 3)
        out.update(metric_alone(model, ds, ids, 20))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
