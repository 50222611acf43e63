#!/usr/bin/env python3
"""Time the autoencoder's run and its two launches.  Three JSON lines; needs the GPU.

Every measure alternates its arms in one process, host clock around a synchronised call, after a warm-up of every arm.
  fit_epoch:  train.fit(max_epochs=1, validate_first=False) with train_autoencoder's settings -- frames gathered in HBM, the
      loss of a step to a device ring, validation_loss on the device (one read-back per pass), the epoch's checkpoint --
      against the loop the package offered before: host-fed batches (a pinned float32 copy of the frames, .cuda() per
      batch), training_step(backward=True) + optimizer_step, float(loss) every step, validation_step(...).item() per
      validation batch at the same points.  The hand loop writes no checkpoint: "checkpoint_ms" times save_checkpoint
      alone and "fit_less_checkpoint_ms" is the comparable figure.
  recon_terms:  spdm_recon_terms against torch.mean((r - t).double() ** 2, dim=(1, 2, 3)) on B frames.
  frames_to_u8:  spdm_frames_to_bytes against torch's mul / round / clamp / permute / to(uint8) recipe and against a plain
      converting copy that moves the same bytes (B x 27648 floats in, B x 27648 bytes out) without changing the layout.

usage: python tools/bench_autoencoder_fit.py [--batch B] [--rows T] [--iters N]"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from state_policy_diffusionmodel_amd.autoencoder import autoencoder
from state_policy_diffusionmodel_amd.dataset import FramesDataModule, frames_to_u8
from state_policy_diffusionmodel_amd.train import fit, validation_points
from state_policy_diffusionmodel_amd.train_metrics import recon_terms_into

SEED = 3


def hand_epoch(model, frames_host, dm, optimizer, batch):
    """the parent's calls only: host-fed batches, a read-back per step and per validation batch"""
    order = dm.train_dataloader(0).row_ids
    n = -(-len(order) // batch)
    points = set(validation_points(n, 0.5))
    losses, vals = [], []
    for i in range(n):
        x = frames_host[torch.as_tensor(order[i * batch:(i + 1) * batch])].cuda()
        loss = model.training_step(x, backward=True)
        model.optimizer_step(optimizer, 0.5)
        losses.append(float(loss))
        if i in points:
            tot, cnt = 0.0, 0
            for j in range(0, len(dm.val_ids), batch):
                vb = frames_host[torch.as_tensor(dm.val_ids[j:j + batch])].cuda()
                tot += model.validation_step(vb).item() * vb.shape[0]
                cnt += vb.shape[0]
            vals.append(tot / cnt)
    return losses, vals


def alternate(arms, iters):
    for fn in arms.values():
        fn()
    ms = {k: [] for k in arms}
    for _ in range(iters):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for k, v in ms.items():
        out[k], out[k.replace("_ms", "_min_ms")] = round(statistics.median(v), 3), round(min(v), 3)
    return out


def main():
    args = sys.argv[1:]
    opt = {"--batch": 128, "--rows": 2560, "--iters": 5}
    for flag in list(opt):
        if flag in args:
            i = args.index(flag)
            opt[flag] = type(opt[flag])(args[i + 1])
            del args[i:i + 2]
    if args:
        raise SystemExit(__doc__)
    if not torch.cuda.is_available():
        raise SystemExit("bench_autoencoder_fit needs the GPU: there is nothing to time without it")
    batch, T, iters = opt["--batch"], opt["--rows"], opt["--iters"]
    img = np.random.default_rng(0).integers(0, 256, (T, 96, 96, 3), dtype=np.uint8)
    dm = FramesDataModule(batch, seed=SEED)
    dm.setup(arrays={"img": img})
    frames_host = (torch.from_numpy(img).permute(0, 3, 1, 2).to(torch.float32) / 255).contiguous().pin_memory()

    a, b = autoencoder(weight_seed=1), autoencoder(weight_seed=1)
    hand_opt = b.configure_optimizers(device_optimizer=True)["optimizer"]
    n_train, n_val = len(dm.train_dataloader(0)), len(dm.val_dataloader())
    with tempfile.TemporaryDirectory() as tmp:
        res = alternate({"fit_ms": lambda: fit(a, dm, max_epochs=1, out_dir=tmp, val_check_interval=0.5, seed=SEED, validate_first=False),
                         "hand_ms": lambda: hand_epoch(b, frames_host, dm, hand_opt, batch),
                         "checkpoint_ms": lambda: a.save_checkpoint(os.path.join(tmp, "alone.ckpt"), optimizer=hand_opt)}, iters)
    out = {"measure": "fit_epoch", "batch_size": batch, "frames": T, "train_batches": n_train, "val_batches": n_val,
           "validations": len(validation_points(n_train, 0.5)), "iters": iters, **res}
    out["fit_less_checkpoint_ms"] = round(out["fit_ms"] - out["checkpoint_ms"], 3)
    out["hand_over_fit_less_checkpoint"] = round(out["hand_ms"] / out["fit_less_checkpoint_ms"], 3)
    print(json.dumps(out), flush=True)

    x = dm.data_full.frames(np.arange(batch))
    r = a.decoder(a.encoder(x))
    terms = torch.empty(batch, dtype=torch.float64, device=x.device)
    reps = 50                                                                  # a launch is microseconds: time 50 in a row

    def many(fn):
        def run():
            for _ in range(reps):
                fn()
        return run

    res = alternate({"hip_ms": many(lambda: recon_terms_into(r, x, terms)),
                     "torch_ms": many(lambda: torch.mean((r - x).double() ** 2, dim=(1, 2, 3)))}, iters)
    rel = float(((terms - torch.mean((r - x).double() ** 2, dim=(1, 2, 3))).abs() / terms).max())
    print(json.dumps({"measure": "recon_terms", "frames": batch, "launches_per_sample": reps, "iters": iters, **res,
                      "torch_over_hip": round(res["torch_ms"] / res["hip_ms"], 3), "max_rel_diff": rel}), flush=True)

    sheet = torch.empty((batch * 96, 96, 3), dtype=torch.uint8, device=x.device)
    planar_bytes = torch.empty(x.shape, dtype=torch.uint8, device=x.device)

    def recipe():
        return (x * 255).round().clamp(0, 255).permute(0, 2, 3, 1).to(torch.uint8).contiguous()

    def plain_copy():                                                          # the same bytes in and out, no layout change, no rounding rule
        planar_bytes.copy_(x)

    res = alternate({"hip_ms": many(lambda: frames_to_u8(x, sheet, cols=1)), "torch_ms": many(recipe), "copy_ms": many(plain_copy)}, iters)
    same = bool(torch.equal(sheet.view(batch, 96, 96, 3), recipe()))
    print(json.dumps({"measure": "frames_to_u8", "frames": batch, "launches_per_sample": reps, "iters": iters, **res,
                      "torch_over_hip": round(res["torch_ms"] / res["hip_ms"], 3), "hip_over_copy": round(res["hip_ms"] / res["copy_ms"], 3),
                      "equals_torch_recipe": same}), flush=True)


if __name__ == "__main__":
    main()
