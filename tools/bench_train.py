#!/usr/bin/env python3
"""Time one training step of UNet_Film_noAttention -- or, with --attention, of UNet_Film with its six SelfAttention blocks
(SpdmEngine(train_attention=True)), or, with --simple, of simple_Unet.py's UNet (SpdmEngine(model='UNet', train_simple=True),
CPU side: tests/simple_unet_ref.py) -- (H = 32, D = 3) at B = 16, 64, 256: the HIP step (spdm_train_loss_grad:
forward, MSE loss, full backward), the ways an optimiser step's weights reach the handle -- a rebuild of the handle from a host
state_dict (SpdmEngine.refresh_weights: handle creation + spdm_load_weights), the in-place update from a device flat tensor
(SpdmEngine.update_weights, synchronised), and a whole optimiser step through the facade (Diffusion_DDPM.optimizer_step:
gradient clip + Adam + update_weights) with torch's optimiser (optimizer_step_ms) and with optim.DeviceAdam
(device_optimizer_step_ms; torch_clip_adam_ms / device_clip_adam_ms: the same two without the weight update; the four
alternate in one run, medians) -- and torch-CPU fp32 autograd of the oracle on 16 threads for the same step
(--no-cpu skips it).  --frames adds raw frames (obs_horizon 10: 10 B frames per step) and the jointly trained observation
encoder: encoder_train_ms (VisionEncoder.train_forward + backward, synchronised), the same encoder's
forward + backward through torch-ROCm autograd on an nn.Sequential (torch_encoder_ms; the two alternate, medians), and
optimizer_step_ms becomes the joint step (clip over both parameters + Adam + both weight updates).  Without --frames also the
head of the step: torch_forward_process_ms (randint + randn_like + add_noise + add_constraints in torch)
against device_forward_process_ms (Diffusion_DDPM.forward_process: one HIP launch), and the whole
training_step(backward=True) on a device-resident batch without and with device_noise (training_step_ms /
training_step_device_noise_ms); the four alternate in one run, each synchronised, medians (and minima, *_min_ms).
--forward-process-only prints just those.  One JSON line per batch size.
usage: python tools/bench_train.py [--attention | --simple] [--frames] [--forward-process-only] [--iters N] [--no-cpu] [B ...]"""
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


def encoder_times(B, iters):
    """(HIP train_forward + backward, torch-ROCm autograd of the same nn.Sequential) in ms, medians of alternating runs."""
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd.vision import VisionEncoder
    nn = torch.nn
    n = B * 10
    enc_sd = make_encoder_state_dict(0)
    enc = VisionEncoder(enc_sd)
    ref = nn.Sequential(nn.Conv2d(3, 16, 2, stride=2, padding=1), nn.ReLU(), nn.Conv2d(16, 32, 2, stride=2), nn.ReLU(),
                        nn.Conv2d(32, 64, 2, stride=2), nn.ReLU(), nn.Flatten(), nn.Linear(64 * 12 * 12, 128))
    ref.load_state_dict(enc_sd, strict=True)
    ref.cuda()
    g = torch.Generator().manual_seed(B)
    frames = torch.rand(n, 3, 96, 96, generator=g).cuda()
    gl = (torch.randn(n, 128, generator=g) / (n * 128)).cuda()

    def hip():
        enc.train_forward(frames)
        enc.backward(gl)

    def torch_rocm():
        for p in ref.parameters():
            p.grad = None
        ref(frames).backward(gl)

    ms = {hip: [], torch_rocm: []}
    for _ in range(3):
        hip()
        torch_rocm()
    for _ in range(max(10, iters)):
        for fn in (hip, torch_rocm):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[fn].append((time.perf_counter() - t0) * 1e3)
    enc.close()
    return statistics.median(ms[hip]), statistics.median(ms[torch_rocm]), enc_sd, frames


def facade_model(sd, B, simple, attention, **kw):
    return Diffusion_DDPM(obs_horizon=10, pred_horizon=H - 10, observation_dim=135, prediction_dim=D, inpaint_horizon=10,
                          model="UNet" if simple else "UNet_Film" if attention else "UNet_FilmnoAttention",
                          state_dict=sd, max_batch=B, train_attention=attention, **kw)


def forward_process_times(m, B, iters):
    """The head of a training step in torch and as the one HIP launch, and the whole training_step(backward=True) without and
    with device_noise: the four alternate, every call synchronised; {name: ms} medians and minima."""
    g = torch.Generator().manual_seed(B + 1)
    T = 32          # windows of obs_horizon 10 + pred_horizon 22 steps; observation_dim 135 = 2 + 1 + 4 + 128
    batch = {"position": torch.randn(B, T, 2, generator=g).cuda(), "action": torch.randn(B, T, 1, generator=g).cuda(),
             "velocity": torch.randn(B, T, 4, generator=g).cuda(), "image_features": torch.randn(B, T, 128, generator=g).cuda()}
    obs = m.prepare_observation_batch(batch)
    x_0 = m.prepare_prediction_vectors(m.prepare_prediction_batch(batch)).unsqueeze(1)
    inp = m.prepare_inpaint_vectors(obs).unsqueeze(1)
    window = torch.cat([inp, x_0], dim=2)
    assert tuple(window.shape) == (B, 1, H, D)

    def torch_fp():
        t = torch.randint(0, m.noise_steps, (B,), device=m.device)
        noise = torch.randn_like(window)
        m.add_constraints(m.noise_scheduler.add_noise(window, noise, t), inp)

    arms = {"torch_forward_process_ms": torch_fp,
            "device_forward_process_ms": lambda: m.forward_process(window, inp, seed=1, step=0),
            "training_step_ms": lambda: m.training_step(batch, backward=True),
            "training_step_device_noise_ms": lambda: m.training_step(batch, backward=True, device_noise=True, seed=1)}
    ms = {k: [] for k in arms}
    for it in range(max(20, iters) + 3):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= 3:     # (three warm-up rounds)
                ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    out.update({k.replace("_ms", "_min_ms"): round(min(v), 4) for k, v in ms.items()})
    return out


def main():
    args = sys.argv[1:]
    iters = 20
    fp_only = "--forward-process-only" in args
    if fp_only:
        args.remove("--forward-process-only")
    frames_opt = "--frames" in args
    if frames_opt:
        args.remove("--frames")
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
    model = "UNet (simple_Unet.py)" if simple else "UNet_Film" if attention else "UNet_Film_noAttention"
    if fp_only:
        for B in batches:
            m = facade_model(sd, B, simple, attention)
            teng = m._train_engine_for(B, H, D)
            print(json.dumps({"model": model, "B": B, "H": H, "D": D, **forward_process_times(m, B, iters)}), flush=True)
            teng.close()
        return
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
        extra = {}
        if frames_opt:
            enc_ms, torch_ms, enc_sd, frames = encoder_times(B, iters)
            extra = {"frames": B * 10, "encoder_train_ms": round(enc_ms, 3), "torch_encoder_ms": round(torch_ms, 3),
                     "vision_encoder_state_dict": enc_sd, "train_vision_encoder": True}
        m = facade_model(sd, B, simple, attention,
                         **{k: extra.pop(k) for k in ("vision_encoder_state_dict", "train_vision_encoder") if k in extra})
        teng = m._train_engine_for(B, H, D)
        # both optimisers over the SAME flat parameter(s), alternating (each keeps its own moments; the weights just wander):
        # torch's clip_grad_norm_ + Adam and optim.DeviceAdam
        opt = m.configure_optimizers()["optimizer"]
        dopt = m.configure_optimizers(device_optimizer=True)["optimizer"]
        params = opt.param_groups[0]["params"]
        p = m.noise_estimator.flat_parameter()

        def set_grads():
            p.grad = teng.loss_and_grad(xd, t, cd, nd, flat=True)[2]
            if frames_opt:      # the joint step: the encoder's gradient is there too
                m.vision_encoder.train_forward(frames)
                m.vision_encoder.backward(cd.reshape(B, 10, 135)[..., -128:].reshape(-1, 128).contiguous() * 1e-4)

        def torch_only():
            torch.nn.utils.clip_grad_norm_(params, 0.5)
            opt.step()

        arms = {"optimizer_step_ms": lambda: m.optimizer_step(opt, 0.5),               # clip + Adam + weight update(s)
                "device_optimizer_step_ms": lambda: m.optimizer_step(dopt, 0.5),
                "torch_clip_adam_ms": torch_only,                                        # ... without the weight update(s)
                "device_clip_adam_ms": lambda: dopt.step(max_norm=0.5)}
        opt_ms = {k: [] for k in arms}
        for it in range(max(10, iters) + 2):
            for k, fn in arms.items():
                set_grads()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= 2:     # (two warm-up rounds)
                    opt_ms[k].append((time.perf_counter() - t0) * 1e3)
        if not frames_opt:
            extra.update(forward_process_times(m, B, iters))
        teng.close()
        cpu = float("nan") if no_cpu else cpu_step(sd, x, t, cond, noise, attention, simple)
        hip = statistics.median(step)
        print(json.dumps({"model": model, "B": B, "H": H, "D": D, "hip_step_ms": round(hip, 3), "hip_step_min_ms": round(min(step), 3),
                          "weight_refresh_ms": round(statistics.median(refresh), 2),
                          "weight_update_ms": round(statistics.median(update), 3),
                          **{k: round(statistics.median(v), 3) for k, v in opt_ms.items()}, **extra, "device_bytes": ws,
                          "cpu_autograd_ms": None if no_cpu else round(cpu, 1), "cpu_threads": 16, "cpu_over_hip": None if no_cpu else round(cpu / hip, 1)}),
              flush=True)


if __name__ == "__main__":
    main()
