#!/usr/bin/env python3
"""Time the device dataset.  One JSON line per (measurement, batch size); needs the GPU.

1. "gather": DeviceDataset.batch (ONE HIP launch, spdm_dataset_gather) against torch-ROCm producing the same tensors from
   the same device stores -- store[rows].permute(0,3,1,2).float().div(255) plus the gathers and the float64 position
   arithmetic of the low-dimensional rows -- for the uint8 and the float32 store.  obs 10 / pred 30 / step 5, frames='obs',
   random windows of a store of --frames frames (default 20000: 553 MB as uint8, larger than every cache).  The arms
   alternate in one process; each call is timed with device events; medians and minima after three warm-up rounds.  bytes =
   what the algorithm must move: per frame 27648 + 110592 (uint8) or 2 x 110592 (float32), plus the low-dimensional rows.
2. "step": training_step(backward=True, device_noise=True) + optimizer_step per batch, the batch (a) from
   DeviceDataset.batch and (b) assembled by numpy on the host (one thread; obs frames only, float32) into pinned memory and
   copied with .to(device).  Host clock around a synchronised step; the two alternate.  h2d_GBps is the rate of that copy.

usage: python tools/bench_dataset.py [--frames T] [--iters N] [--no-step] [B ...]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from state_policy_diffusionmodel_amd.dataset import DeviceDataset
from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM

OBS, PRED, STEP, EPISODE = 10, 30, 5, 1000
PEAK_BPS = 8e12            # the HBM figure the README's roofline uses


def make_arrays(T):
    rng = np.random.default_rng(0)
    return {"position": 30.0 * rng.standard_normal((T, 2)), "velocity": rng.standard_normal((T, 2)), "action": rng.uniform(-1, 1, (T, 3)),
            "img": rng.integers(0, 256, (T, 96, 96, 3), dtype=np.uint8), "ends": np.arange(EPISODE, T + 1, EPISODE)}


def torch_batch(ds, ids):
    """The same four tensors with torch-ROCm ops on the same device stores."""
    seq = OBS + PRED
    start = ds._d_start[ids.long()].long()
    rows = start[:, None] + STEP * torch.arange(seq, device=ids.device)
    img = ds._img[rows[:, :OBS].reshape(-1)].permute(0, 3, 1, 2).float()
    if ds.image_storage == "uint8":
        img = img.div(255)
    sn = (ds._position[rows] - ds._pos_min) / (ds._pos_max - ds._pos_min) * 2 - 1
    return {"image": img.view(len(ids), OBS, 3, 96, 96), "position": ((sn - sn[:, :1]) / 2.0).float(),
            "velocity": ds._velocity[rows], "action": ds._action[rows]}


def gather_times(sets, B, iters):
    n = len(sets["uint8"])
    g = torch.Generator().manual_seed(B)
    ids = [torch.randint(0, n, (B,), generator=g).to(torch.int32).cuda() for _ in range(iters + 3)]
    arms = {}
    for name, ds in sets.items():
        arms[f"hip_{name}"] = (lambda i, ds=ds: ds.batch(ids[i]))
        arms[f"torch_{name}"] = (lambda i, ds=ds: torch_batch(ds, ids[i]))
    bit_equal = {}
    for name, ds in sets.items():           # the two arms agree before either is timed
        a, b = arms[f"hip_{name}"](0), arms[f"torch_{name}"](0)
        assert torch.allclose(a["image"], b["image"], rtol=0, atol=1e-7) and torch.equal(a["velocity"], b["velocity"])
        bit_equal[name] = bool(torch.equal(a["image"], b["image"]))      # torch may multiply by 1 / 255 where the kernel divides
        assert torch.allclose(a["position"], b["position"], rtol=0, atol=1e-6)
    us = {k: [] for k in arms}
    for it in range(iters + 3):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn(it)
            e1.record()
            e1.synchronize()
            if it >= 3:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    low = B * (OBS + PRED) * (2 * 8 + 2 * 4 + 3 * 4 + 7 * 4)
    out = {"measure": "gather", "B": B, "frames_per_batch": B * OBS, "store_frames": sets["uint8"]._T, "iters": iters}
    for k, v in us.items():
        per = 27648 + 110592 if k.endswith("uint8") else 2 * 110592
        med = statistics.median(v)
        out[k + "_us"], out[k + "_min_us"] = round(med, 2), round(min(v), 2)
        if k.startswith("hip_"):
            bps = (B * OBS * per + low) / (med * 1e-6)
            out[k + "_TBps"], out[k + "_of_peak"] = round(bps / 1e12, 3), round(bps / PEAK_BPS, 3)
    for name in sets:
        out[f"torch_over_hip_{name}"] = round(out[f"torch_{name}_us"] / out[f"hip_{name}_us"], 3)
        out[f"torch_image_bit_equal_{name}"] = bit_equal[name]
    return out


def step_times(ds, arrays, img_f32, B, iters):
    from oracle.encoder_ref import make_encoder_state_dict
    m = Diffusion_DDPM(model="UNet_FilmnoAttention", obs_horizon=OBS, pred_horizon=PRED, inpaint_horizon=OBS, observation_dim=135,
                       prediction_dim=5, vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=B)
    opt = m.configure_optimizers(device_optimizer=True)["optimizer"]
    seq = OBS + PRED
    nvel = np.ascontiguousarray(ds._velocity.cpu().numpy())
    nact = np.ascontiguousarray(ds._action.cpu().numpy())
    pos, lo, hi = arrays["position"], ds._pos_min, ds._pos_max
    pinned = {"image": torch.empty((B, OBS, 3, 96, 96), dtype=torch.float32).pin_memory(),
              "position": torch.empty((B, seq, 2), dtype=torch.float32).pin_memory(),
              "velocity": torch.empty((B, seq, 2), dtype=torch.float32).pin_memory(),
              "action": torch.empty((B, seq, 3), dtype=torch.float32).pin_memory()}
    views = {k: v.numpy() for k, v in pinned.items()}
    g = torch.Generator().manual_seed(B + 7)
    ids = [torch.randint(0, len(ds), (B,), generator=g) for _ in range(iters + 2)]
    h2d = []

    def host_batch(i):
        for b, w in enumerate(ids[i].tolist()):
            s = int(ds.indices[w, 0])
            rows = slice(s, s + seq * STEP, STEP)
            views["image"][b] = np.moveaxis(img_f32[s:s + OBS * STEP:STEP], -1, 1)
            sn = (pos[rows] - lo) / (hi - lo) * 2 - 1
            views["position"][b] = (sn - sn[0]) / 2.0
            views["velocity"][b], views["action"][b] = nvel[rows], nact[rows]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = {k: v.to(ds.device) for k, v in pinned.items()}
        torch.cuda.synchronize()
        h2d.append(sum(v.numel() * 4 for v in pinned.values()) / (time.perf_counter() - t0))
        return out

    d_ids = [i.to(torch.int32).cuda() for i in ids]
    arms = {"step_device_dataset_ms": lambda i: ds.batch(d_ids[i]), "step_host_batch_ms": host_batch}
    ms = {k: [] for k in arms}
    for it in range(iters + 2):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.training_step(fn(it), backward=True, device_noise=True, seed=1)
            m.optimizer_step(opt)
            torch.cuda.synchronize()
            if it >= 2:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"measure": "step", "B": B, "H": OBS + PRED, "D": 5, "iters": iters}
    for k, v in ms.items():
        out[k], out[k.replace("_ms", "_min_ms")] = round(statistics.median(v), 3), round(min(v), 3)
    out["h2d_GBps"] = round(statistics.median(h2d[2:]) / 1e9, 2)
    out["host_batch_MB"] = round(sum(v.numel() * 4 for v in pinned.values()) / 1e6, 1)
    return out


def main():
    args = sys.argv[1:]
    T, iters, do_step = 20000, 30, True
    if "--frames" in args:
        i = args.index("--frames")
        T = int(args[i + 1])
        del args[i:i + 2]
    if "--iters" in args:
        i = args.index("--iters")
        iters = int(args[i + 1])
        del args[i:i + 2]
    if "--no-step" in args:
        args.remove("--no-step")
        do_step = False
    sizes = [int(a) for a in args] or [16, 64, 256]
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset needs the GPU: there is nothing to time without it")
    arrays = make_arrays(T)
    img_f32 = np.empty((T, 96, 96, 3), np.float32)
    for i in range(0, T, 512):
        img_f32[i:i + 512] = arrays["img"][i:i + 512] / np.float32(255)
    mk = lambda img, st: DeviceDataset(arrays["position"], arrays["velocity"], arrays["action"], img, arrays["ends"], PRED, OBS,  # noqa: E731
                                       step_size=STEP, image_storage=st)
    sets = {"uint8": mk(arrays["img"], "auto"), "float32": mk(img_f32, "float32")}
    for B in sizes:
        print(json.dumps(gather_times(sets, B, iters)), flush=True)
    del sets["float32"]
    torch.cuda.empty_cache()
    if do_step:
        for B in sizes:
            print(json.dumps(step_times(sets["uint8"], arrays, img_f32, B, max(4, iters // (1 + B // 32)))), flush=True)


if __name__ == "__main__":
    main()
