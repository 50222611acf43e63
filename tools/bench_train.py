#!/usr/bin/env python3
"""Time one training step of UNet_Film_noAttention -- or, with --attention, of UNet_Film with its six SelfAttention blocks
(SpdmEngine(train_attention=True)), or, with --simple, of simple_Unet.py's UNet (SpdmEngine(model='UNet', train_simple=True),
CPU side: tests/simple_unet_ref.py) -- (H = 32, D = 3) at B = 16, 64, 256: the HIP step (spdm_train_loss_grad:
forward, MSE loss, full backward), the ways an optimiser step's weights reach the handle -- a rebuild of the handle from a host
state_dict (SpdmEngine.refresh_weights: handle creation + spdm_load_weights), the in-place update from a device flat tensor
(SpdmEngine.update_weights, synchronised), and a whole optimiser step through the facade (Diffusion_DDPM.optimizer_step:
gradient clip + Adam + update_weights) -- and torch-CPU fp32 autograd of the oracle on 16 threads for the same step
(--no-cpu skips it).  One JSON line per batch size.
usage: python tools/bench_train.py [--attention | --simple] [--iters N] [--no-cpu] [B ...]"""
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

from oracle.unet_film_ref import unet_film_forward
from simple_unet_ref import simple_unet_forward
from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
from state_policy_diffusionmodel_amd.engine import SpdmEngine
from state_policy_diffusionmodel_amd.weights import random_state_dict

H, D, COND = 32, 3, 1350


def cpu_step(sd, x, t, cond, noise, attention, simple=False):
    params = {k: torch.from_numpy(np.asarray(v)).requires_grad_(k != "pos_encoding.pos_encoding") for k, v in sd.items()}
    fwd = getattr(unet_film_forward, "__wrapped__", unet_film_forward)
    if simple:
        sfwd = getattr(simple_unet_forward, "__wrapped__", simple_unet_forward)
        fwd = lambda p, x, t, c, attention: sfwd(p, x, t, c)       # noqa: E731
    t0 = time.perf_counter()
    with torch.enable_grad():
        loss = torch.mean((noise - fwd(params, x, t, cond, attention=attention)) ** 2)
        loss.backward()
    return (time.perf_counter() - t0) * 1e3


def main():
    args = sys.argv[1:]
    iters = 20
    attention = "--attention" in args
    if attention:
        args.remove("--attention")
    simple = "--simple" in args
    if simple:
        args.remove("--simple")
    no_cpu = "--no-cpu" in args
    if no_cpu:
        args.remove("--no-cpu")
    if "--iters" in args:
        i = args.index("--iters")
        iters = int(args[i + 1])
        del args[i:i + 2]
    batches = [int(a) for a in args] or [16, 64, 256]
    torch.set_num_threads(16)
    sd = (random_state_dict(COND, seed=0, model="UNet", noise_steps=1000) if simple else
          random_state_dict(COND, seed=0, attention=attention))
    for B in batches:
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, 1, H, D, generator=g)
        noise = torch.randn(B, 1, H, D, generator=g)
        cond = torch.randn(B, 1, 10, 135, generator=g)
        t = torch.randint(0, 1000, (B,), generator=g)
        if simple:
            eng = SpdmEngine(H, D, COND, max_batch=B, model="UNet", num_train_timesteps=1001, train_simple=True)
        else:
            eng = SpdmEngine(H, D, COND, max_batch=B, attention=attention, train=True, train_attention=attention)
        eng.load_state_dict(sd)
        xd, nd, cd = x.cuda(), noise.cuda(), cond.cuda()
        for _ in range(3):
            eng.loss_and_grad(xd, t, cd, nd, flat=True)
        torch.cuda.synchronize()
        step = []
        for _ in range(iters):
            t0 = time.perf_counter()
            eng.loss_and_grad(xd, t, cd, nd, flat=True)
            torch.cuda.synchronize()
            step.append((time.perf_counter() - t0) * 1e3)
        refresh = []
        for _ in range(max(3, iters // 4)):
            t0 = time.perf_counter()
            eng.refresh_weights(sd)
            torch.cuda.synchronize()
            refresh.append((time.perf_counter() - t0) * 1e3)
        flat = eng.pack_weights(sd)
        update = []
        for _ in range(max(5, iters)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.update_weights(flat)
            torch.cuda.synchronize()
            update.append((time.perf_counter() - t0) * 1e3)
        ws = eng.device_bytes
        eng.close()
        # a whole optimiser step through the facade: clip + Adam over the flat parameter + update_weights of its engines
        m = Diffusion_DDPM(obs_horizon=10, pred_horizon=H - 10, observation_dim=135, prediction_dim=D, inpaint_horizon=10,
                           model="UNet" if simple else "UNet_Film" if attention else "UNet_FilmnoAttention",
                           state_dict=sd, max_batch=B, train_attention=attention)
        teng = m._train_engine_for(B, H, D)
        opt = m.configure_optimizers()["optimizer"]
        p = m.noise_estimator.flat_parameter()
        opt_ms = []
        for _ in range(max(5, iters)):
            p.grad = teng.loss_and_grad(xd, t, cd, nd, flat=True)[2]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.optimizer_step(opt, 0.5)
            torch.cuda.synchronize()
            opt_ms.append((time.perf_counter() - t0) * 1e3)
        teng.close()
        cpu = float("nan") if no_cpu else cpu_step(sd, x, t, cond, noise, attention, simple)
        hip = statistics.median(step)
        model = "UNet (simple_Unet.py)" if simple else "UNet_Film" if attention else "UNet_Film_noAttention"
        print(json.dumps({"model": model, "B": B, "H": H, "D": D, "hip_step_ms": round(hip, 3), "hip_step_min_ms": round(min(step), 3),
                          "weight_refresh_ms": round(statistics.median(refresh), 2),
                          "weight_update_ms": round(statistics.median(update), 3),
                          "optimizer_step_ms": round(statistics.median(opt_ms), 3), "device_bytes": ws,
                          "cpu_autograd_ms": None if no_cpu else round(cpu, 1), "cpu_threads": 16, "cpu_over_hip": None if no_cpu else round(cpu / hip, 1)}),
              flush=True)


if __name__ == "__main__":
    main()
