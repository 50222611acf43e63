#!/usr/bin/env python3
"""Time the EMA of the weights.  Three JSON lines, printed and written to --out; needs the GPU.

All arms of a measure alternate in one process; a sample is a host clock around ``--reps`` calls that end in a device
synchronise; medians and minima over ``--iters`` samples.
  (a) launch:          spdm_ema_step over model='UNet_Film''s blob (12 bytes per weight: ema read and written, p read) against
                       a plain device copy that moves the same number of bytes (ratio, as DESIGN 8.13 / 8.14 report theirs),
                       torch's ``shadow.sub_((shadow - p) * omd)`` and its ``torch._foreach`` form.
  (b) optimizer_step:  with an EMA configured, without one, and the parent commit's body of the method restated below
                       (``parent_optimizer_step``: the baseline), all on the same model and gradients.
  (c) validation_loss: with ``use_ema=True`` against without -- the price of the two weight swaps.

usage: python tools/bench_ema.py [--batch B] [--iters N] [--reps R] [--val_batches V] [--out PATH]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
from state_policy_diffusionmodel_amd.optim import DeviceEMA

OBS, PRED, INP, D = 2, 30, 2, 5


def parent_optimizer_step(model, optimizer, gradient_clip_val):
    """Diffusion_DDPM.optimizer_step's DeviceAdam branch as it stood before the EMA existed."""
    optimizer.step(max_norm=gradient_clip_val or None)
    model.noise_estimator.mark_moved()
    model.noise_estimator._push()


def timed(arms, iters, reps):
    for fn in arms.values():                                                  # warm-up: code objects, allocations
        fn()
    ms = {k: [] for k in arms}
    for _ in range(iters):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / reps)
    out = {}
    for k, v in ms.items():
        out[k + "_ms"], out[k + "_min_ms"] = round(statistics.median(v), 4), round(min(v), 4)
    return out


def batch_of(B, gen):
    T = OBS + PRED
    return {"position": torch.randn(B, T, 2, generator=gen), "action": torch.randn(B, T, 3, generator=gen),
            "velocity": torch.randn(B, T, 2, generator=gen), "image_features": torch.randn(B, T, 128, generator=gen)}


def main():
    args = sys.argv[1:]
    opt = {"--batch": 64, "--iters": 7, "--reps": 20, "--val_batches": 4, "--out": os.path.join(ROOT, "profiles", "ema_bench.jsonl")}
    for flag in list(opt):
        if flag in args:
            i = args.index(flag)
            opt[flag] = type(opt[flag])(args[i + 1])
            del args[i:i + 2]
    if args:
        raise SystemExit(__doc__)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema needs the GPU: there is nothing to time without it")
    B, iters, reps = opt["--batch"], opt["--iters"], opt["--reps"]
    gen = torch.Generator().manual_seed(0)

    def make():
        return Diffusion_DDPM(noise_steps=1000, obs_horizon=OBS, pred_horizon=PRED, observation_dim=135, prediction_dim=D,
                              model="UNet_Film", inpaint_horizon=INP, weight_seed=1, max_batch=B, train_attention=True)

    lines = []
    # ---- (a) the launch alone -----------------------------------------------------------------------------------------------
    plain, averaged = make(), make()
    p = plain.noise_estimator.flat_parameter()
    n = p.numel()
    moving = torch.nn.Parameter(p.detach().clone() + 1e-3)
    ema = DeviceEMA([moving], min_value=0.999, max_value=0.999)
    ema.step()                                                                # (the first update copies: decay 0)
    shadow_t, shadow_f = ema.shadow[0].clone(), ema.shadow[0].clone()
    omd = 1.0 - 0.999
    words = n * 12 // 8                                                       # a copy reads and writes: the same bytes in all
    src, dst = torch.empty(words, device="cuda"), torch.empty(words, device="cuda")
    q = moving.detach()
    a = timed({"ema_step": ema.step,
               "copy_same_bytes": lambda: dst.copy_(src),
               "torch_sub": lambda: shadow_t.sub_((shadow_t - q) * omd),
               "torch_foreach": lambda: torch._foreach_sub_([shadow_f], torch._foreach_mul(torch._foreach_sub([shadow_f], [q]), omd))},
              iters, reps)
    a = dict({"measure": "ema_launch", "model": "UNet_Film", "weights": n, "bytes_moved": 12 * n, "iters": iters, "reps": reps}, **a)
    a["gb_per_s"] = round(12 * n / a["ema_step_ms"] / 1e6, 1)
    a["ema_over_copy"] = round(a["ema_step_ms"] / a["copy_same_bytes_ms"], 3)
    a["torch_sub_over_ema"] = round(a["torch_sub_ms"] / a["ema_step_ms"], 3)
    a["torch_foreach_over_ema"] = round(a["torch_foreach_ms"] / a["ema_step_ms"], 3)
    lines.append(a)
    del src, dst, shadow_t, shadow_f, ema, moving

    # ---- (b) optimizer_step ---------------------------------------------------------------------------------------------------
    batch = batch_of(B, gen)
    opts = {}
    for name, m in (("plain", plain), ("averaged", averaged)):
        opts[name] = m.configure_optimizers(device_optimizer=True)["optimizer"]
        m.training_step({k: v.clone() for k, v in batch.items()}, backward=True, device_noise=True, seed=1, noise_step=0)
    averaged.configure_ema()
    b = timed({"parent_body": lambda: parent_optimizer_step(plain, opts["plain"], 0.5),
               "without_ema": lambda: plain.optimizer_step(opts["plain"], 0.5),
               "with_ema": lambda: averaged.optimizer_step(opts["averaged"], 0.5)}, iters, reps)
    b = dict({"measure": "optimizer_step", "model": "UNet_Film", "batch_size": B, "weights": n, "iters": iters, "reps": reps}, **b)
    b["without_over_parent"] = round(b["without_ema_ms"] / b["parent_body_ms"], 3)
    b["with_over_parent"] = round(b["with_ema_ms"] / b["parent_body_ms"], 3)
    b["ema_added_ms"] = round(b["with_ema_ms"] - b["parent_body_ms"], 4)
    lines.append(b)

    # ---- (c) validation_loss ---------------------------------------------------------------------------------------------------
    batches = [batch_of(B, gen) for _ in range(opt["--val_batches"])]
    vreps = max(1, reps // 10)
    c = timed({"live": lambda: averaged.validation_loss(batches, seed=1),
               "use_ema": lambda: averaged.validation_loss(batches, seed=1, use_ema=True)}, iters, vreps)
    c = dict({"measure": "validation_loss", "model": "UNet_Film", "batch_size": B, "val_batches": len(batches), "iters": iters,
              "reps": vreps}, **c)
    c["swap_cost_ms"] = round(c["use_ema_ms"] - c["live_ms"], 4)
    c["use_ema_over_live"] = round(c["use_ema_ms"] / c["live_ms"], 3)
    lines.append(c)

    os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
    with open(opt["--out"], "w") as fh:
        for line in lines:
            print(json.dumps(line), flush=True)
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
