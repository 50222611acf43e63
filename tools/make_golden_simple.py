#!/usr/bin/env python3
"""Generate the golden vectors of the concat-conditioned U-Net (the reference's ``models/simple_Unet.py``, built by
``Diffusion_DDPM(model='UNet')``) under tests/golden/:

    simple_inventory.json                 state_dict names and shapes of the reference module at two cond_dims
    simple_unet_h{H}d{D}_b{B}.npz         eps at a scalar t and at a per-sample t, with the weights' sha256
    simple_traj_{ddpm,ddim}_*.npz         every iterate of a DDPM (in-painting 4 rows) and a DDIM loop, pre-drawn noise

Runs only where the reference checkout is available.  Like tools/make_golden.py, it imports the reference module,
loads OUR deterministic weights into it (``random_state_dict(..., model='UNet')``, ``load_state_dict(strict=True)``
pins the inventory), evaluates it in eval mode and stores inputs and outputs.  Trajectories are the oracle's loop
(oracle/scheduler_ref.py) driving the imported reference network.  Only data is written; weights are regenerated from
the seed by the tests and checked against the stored hash.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle.scheduler_ref import sample_loop
from state_policy_diffusionmodel_amd.weights import blob_sha256, random_state_dict

REF = os.environ.get("SPDM_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
NOISE_STEPS = 1000
OBS_H, OBS_DIM = 10, 2          # Diffusion_DDPM's defaults: cond_dim 20


def import_reference():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from models.simple_Unet import UNet
    return UNet


def build_reference_model(cond_dim, seed):
    UNet = import_reference()
    m = UNet(in_channels=1, out_channels=1, noise_steps=NOISE_STEPS, time_dim=256, global_cond_dim=cond_dim)
    sd = random_state_dict(cond_dim, seed=seed, model="UNet", noise_steps=NOISE_STEPS)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.eval()                    # PositionalEncoding's dropout off: sampling semantics
    return m, sd


def gen(seed):
    return torch.Generator().manual_seed(seed)


def inventory_case():
    UNet = import_reference()
    inv = {}
    for cd in (20, 1350):
        m = UNet(1, 1, NOISE_STEPS, time_dim=256, global_cond_dim=cd)
        inv[f"cond_dim_{cd}"] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    path = os.path.join(OUT, "simple_inventory.json")
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(f'"{key}": [\n' + ",\n".join(json.dumps(e) for e in entries) + "\n]"
                                    for key, entries in inv.items()) + "\n}\n")
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def forward_case(H, D, B, wseed=0):
    cond_dim = OBS_H * OBS_DIM
    m, sd = build_reference_model(cond_dim, wseed)
    x = torch.randn(B, 1, H, D, generator=gen(300 + H * 10 + D))
    y = torch.randn(B, 1, OBS_H, OBS_DIM, generator=gen(400 + B))
    t0 = torch.tensor([637], dtype=torch.int64)
    t1 = (torch.arange(B, dtype=torch.int64) * 331 + 5) % (NOISE_STEPS + 1)
    out = {"x": x.numpy(), "cond": y.numpy(), "H": H, "D": D, "B": B, "obs_h": OBS_H, "obs_dim": OBS_DIM,
           "noise_steps": NOISE_STEPS, "wseed": wseed, "weights_sha256": blob_sha256(sd)}
    with torch.no_grad():
        for i, t in enumerate((t0, t1)):
            out[f"t{i}"] = t.numpy()
            out[f"eps{i}"] = m(x, t, y).numpy()
    path = os.path.join(OUT, f"simple_unet_h{H}d{D}_b{B}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def trajectory_case(name, kind, T, N, H, D, B, inp_h, wseed=0):
    cond_dim = OBS_H * OBS_DIM
    m, sd = build_reference_model(cond_dim, wseed)
    x_T = torch.rand(B, 1, H, D, generator=gen(12))
    cond = torch.randn(B, 1, OBS_H, OBS_DIM, generator=gen(11))
    noise = torch.randn(N, B, 1, H, D, generator=gen(13))
    inpaint = torch.rand(B, 1, inp_h, D, generator=gen(14)) * 2 - 1 if inp_h > 0 else None
    with torch.no_grad():
        hist = sample_loop(lambda x, t, y: m(x, t, y), kind, T, N, cond, x_T,
                           noise if kind == "ddpm" else None, inpaint, history=True)
    out = {"kind": kind, "T": T, "N": N, "H": H, "D": D, "B": B, "obs_h": OBS_H, "obs_dim": OBS_DIM,
           "inp_h": inp_h, "noise_steps": NOISE_STEPS, "wseed": wseed, "weights_sha256": blob_sha256(sd),
           "x_T": x_T.numpy(), "cond": cond.numpy(), "noise": noise.numpy(),
           "history": np.stack([h.numpy() for h in hist])}
    if inpaint is not None:
        out["inpaint"] = inpaint.numpy()
    path = os.path.join(OUT, f"simple_traj_{name}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    inventory_case()
    for H, D, B in ((32, 3, 2), (16, 3, 1), (31, 5, 2), (64, 6, 1), (8, 1, 2)):
        forward_case(H, D, B)
    trajectory_case("ddpm_T20_h16d3_b2_inp4", "ddpm", 20, 20, 16, 3, 2, inp_h=4)
    trajectory_case("ddim_T10_h16d3_b2", "ddim", 10, 10, 16, 3, 2, inp_h=0)


if __name__ == "__main__":
    main()
