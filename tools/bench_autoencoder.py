#!/usr/bin/env python3
"""Time one reconstruction-training step of the autoencoder at n = 16, 128 (the reference's batch) and
512 frames: the HIP step -- autoencoder.training_step(backward=True) + optimizer_step (global-norm clip 0.5, Adam, both
in-place weight updates) -- against torch-ROCm autograd of the same two nn.Sequentials with the same clip and Adam.  The
two alternate on one device, each run synchronised; medians of 10.  Also the HIP step's parts (encoder forward, decoder
loss, decoder backward, encoder backward, optimiser step), each synchronised, as shares of their sum, and the optimiser step with both optimisers on
the same gradients in the same run: torch's clip + Adam (optimizer_step_ms, the one in the parts) and optim.DeviceAdam
(device_optimizer_step_ms), both including the two in-place weight updates.
One JSON line per n.
usage: python tools/bench_autoencoder.py [--iters N] [n ...]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from state_policy_diffusionmodel_amd.autoencoder import autoencoder


def torch_modules(sd):
    nn = torch.nn
    enc = nn.Sequential(nn.Conv2d(3, 16, 2, stride=2, padding=1), nn.ReLU(), nn.Conv2d(16, 32, 2, stride=2), nn.ReLU(),
                        nn.Conv2d(32, 64, 2, stride=2), nn.ReLU(), nn.Flatten(), nn.Linear(64 * 12 * 12, 128))
    dec = nn.Sequential(nn.Linear(128, 64 * 12 * 12), nn.Unflatten(1, (64, 12, 12)), nn.ConvTranspose2d(64, 32, 2, stride=2),
                        nn.ReLU(), nn.ConvTranspose2d(32, 16, 2, stride=2), nn.ReLU(), nn.ConvTranspose2d(16, 3, 2, stride=2),
                        nn.Sigmoid())
    enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, strict=True)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=True)
    return enc.cuda(), dec.cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bench(n, iters):
    torch.manual_seed(n)
    ae = autoencoder(learning_rate=1e-3)
    enc, dec = torch_modules(ae.state_dict())
    params = list(enc.parameters()) + list(dec.parameters())
    ref_opt = torch.optim.Adam(params, lr=1e-3)
    opt = ae.configure_optimizers()["optimizer"]
    dopt = ae.configure_optimizers(device_optimizer=True)["optimizer"]       # optim.DeviceAdam over the same two parameters
    x = torch.rand(n, 3, 96, 96, generator=torch.Generator().manual_seed(n)).cuda()

    def hip():
        ae.training_step(x, backward=True)
        ae.optimizer_step(opt, 0.5)

    def torch_rocm():
        ref_opt.zero_grad(set_to_none=True)
        torch.mean((dec(enc(x)) - x) ** 2).backward()
        torch.nn.utils.clip_grad_norm_(params, 0.5)
        ref_opt.step()

    ms = {hip: [], torch_rocm: []}
    for _ in range(3):
        hip()
        torch_rocm()
    for _ in range(iters):
        for fn in (hip, torch_rocm):
            ms[fn].append(timed(fn))
    # the HIP step's parts, each synchronised (their sum exceeds the step by the extra synchronisations)
    parts = {k: [] for k in ("encoder_forward", "decoder_loss", "decoder_backward", "encoder_backward", "optimizer_step")}
    dev_opt = []
    for it in range(iters):
        state = {}
        parts["encoder_forward"].append(timed(lambda: state.update(z=ae.encoder.train_forward(x))))
        parts["decoder_loss"].append(timed(lambda: ae.decoder.train_loss(state["z"], x)))
        parts["decoder_backward"].append(timed(lambda: state.update(gl=ae.decoder.backward()[1])))
        parts["encoder_backward"].append(timed(lambda: ae.encoder.backward(state["gl"])))
        # both optimisers on this step's gradients, in alternating order (each keeps its own moments)
        for which in ((opt, dopt) if it % 2 == 0 else (dopt, opt)):
            (parts["optimizer_step"] if which is opt else dev_opt).append(timed(lambda: ae.optimizer_step(which, 0.5)))
    med = {k: statistics.median(v) for k, v in parts.items()}
    total = sum(med.values())
    h, t = statistics.median(ms[hip]), statistics.median(ms[torch_rocm])
    ae.close()
    return {"n": n, "hip_step_ms": round(h, 3), "torch_rocm_step_ms": round(t, 3), "hip_over_torch": round(h / t, 2),
            "optimizer_step_ms": round(med["optimizer_step"], 3), "device_optimizer_step_ms": round(statistics.median(dev_opt), 3),
            "parts_ms": {k: round(v, 3) for k, v in med.items()}, "parts_share": {k: round(v / total, 3) for k, v in med.items()}}


def main():
    args = sys.argv[1:]
    iters = 10
    if "--iters" in args:
        i = args.index("--iters")
        iters = int(args[i + 1])
        del args[i:i + 2]
    for n in [int(a) for a in args] or [16, 128, 512]:
        print(json.dumps(bench(n, iters)), flush=True)


if __name__ == "__main__":
    main()
