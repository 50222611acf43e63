#!/usr/bin/env python3
"""Record the training-gradient fixture tests/golden/train_grad_h16d3_b2.npz (--attention: train_grad_attn_h16d3_b2.npz,
--simple: train_grad_simple_h16d3_b2.npz).

Runs ONLY in the build container (needs /root/reference).  It imports the reference module
UNet_Film_noAttention (models/Unet_FiLmLayer_noAttention.py, with a stub for the unused top-level
`import torchvision`), loads OUR deterministic generated weights into it (strict=True), evaluates, in float64,
one training step's loss on seeded inputs -- loss = mean((noise - model(x_noisy, t, cond))^2), per-sample t -- then
loss.backward().  With --attention the module is UNet_Film (models/Unet_FiLmLayer.py, six SelfAttention blocks) and
the fixture is read by tests/test_train_grad_attn_reference.py.  With --simple the module is simple_Unet.py's UNet (the
reference's default network) with our model='UNet' weights, recorded twice: in eval mode (no dropout; keys as above) and with
its PositionalEncoding's dropout replaced by a fixed seeded mask multiply (keys prefixed "drop/", the mask stored as
"drop/scale"); tests/test_train_grad_simple_reference.py reads it.  Stored: the inputs, the loss, d loss / d cond, and for every parameter the gradient's L2 norm, its sum
and 256 elements at seeded flat indices.  Only data is written (tests/test_train_grad_reference.py reads it).
"""
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from state_policy_diffusionmodel_amd.weights import blob_sha256, random_state_dict

REF = "/root/reference"
ATTENTION = "--attention" in sys.argv[1:]
SIMPLE = "--simple" in sys.argv[1:]
OUT = os.path.join(ROOT, "tests", "golden", "train_grad_simple_h16d3_b2.npz" if SIMPLE else
                   "train_grad_attn_h16d3_b2.npz" if ATTENTION else "train_grad_h16d3_b2.npz")
SIMPLE_NOISE_STEPS = 1000
B, H, D, OBS_H, OBS_DIM, WSEED, N_SAMPLES = 2, 16, 3, 2, 7, 21, 256


def sample_indices(name: str, numel: int) -> np.ndarray:
    """256 flat indices of a tensor, seeded by its name (the test draws the same ones)."""
    seed = int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little") ^ numel
    return np.random.default_rng(seed).integers(0, numel, N_SAMPLES)


class _MaskMultiply(torch.nn.Module):
    """Stands in for PositionalEncoding's nn.Dropout: a fixed (B, time_dim) multiplier, the mask over (1 - p)."""

    def __init__(self, scale):
        super().__init__()
        self.scale = scale

    def forward(self, x):
        return x * self.scale


def record(m, x, noise, cond, t, prefix, out):
    """One float64 loss + backward through module m; the statistics of every parameter's gradient under `prefix`."""
    for p in m.parameters():
        p.grad = None
    c = cond.clone().requires_grad_(True)
    loss = torch.mean((noise - m(x, t, c)) ** 2)
    loss.backward()
    out[prefix + "loss"] = loss.item()
    out[prefix + "grad_cond"] = c.grad.numpy()
    names = []
    for name, p in m.named_parameters():
        gr = p.grad.detach().reshape(-1).numpy()
        names.append(name)
        out[f"{prefix}norm/{name}"] = np.linalg.norm(gr)
        out[f"{prefix}sum/{name}"] = gr.sum()
        out[f"{prefix}samp/{name}"] = gr[sample_indices(name, gr.size)]
    out[prefix + "names"] = np.array(names)
    return loss.item(), names


def main_simple():
    sys.path.insert(0, REF)
    from models.simple_Unet import UNet
    cond_dim = OBS_H * OBS_DIM
    torch.set_default_dtype(torch.float64)
    m = UNet(in_channels=1, out_channels=1, noise_steps=SIMPLE_NOISE_STEPS, time_dim=256, global_cond_dim=cond_dim)
    sd = random_state_dict(cond_dim, seed=WSEED, model="UNet", noise_steps=SIMPLE_NOISE_STEPS)
    m.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=True)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, 1, H, D, generator=g, dtype=torch.float64)
    noise = torch.randn(B, 1, H, D, generator=g, dtype=torch.float64)
    cond = torch.randn(B, 1, OBS_H, OBS_DIM, generator=g, dtype=torch.float64)
    t = torch.randint(0, SIMPLE_NOISE_STEPS + 1, (B,), generator=g)
    scale = (torch.rand(B, 256, generator=g, dtype=torch.float64) >= 0.1).double() / 0.9
    out = {"x": x.numpy(), "noise": noise.numpy(), "cond": cond.numpy(), "t": t.numpy(), "wseed": WSEED,
           "noise_steps": SIMPLE_NOISE_STEPS, "weights_sha256": blob_sha256(sd), "drop/scale": scale.numpy()}
    m.eval()                                   # no dropout
    l0, names = record(m, x, noise, cond, t, "", out)
    m.pos_encoding.dropout = _MaskMultiply(scale)
    m.pos_encoding.apply_dropout = True
    l1, _ = record(m, x, noise, cond, t, "drop/", out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(names), "tensors, loss", l0, "(eval),", l1, "(mask)")


def main():
    if SIMPLE:
        return main_simple()
    if "torchvision" not in sys.modules:
        sys.modules["torchvision"] = types.ModuleType("torchvision")
    sys.path.insert(0, REF)
    if ATTENTION:
        from models.Unet_FiLmLayer import UNet_Film as Net
    else:
        from models.Unet_FiLmLayer_noAttention import UNet_Film_noAttention as Net
    cond_dim = OBS_H * OBS_DIM
    # float64 throughout: with float64 as the default dtype the time encoding's frequencies are float64 too (its input,
    # t.float(), holds exact integers), and so is every parameter
    torch.set_default_dtype(torch.float64)
    m = Net(in_channels=1, out_channels=1, noise_steps=1000, time_dim=256, global_cond_dim=cond_dim)
    sd = random_state_dict(cond_dim, seed=WSEED, attention=ATTENTION)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, 1, H, D, generator=g, dtype=torch.float64)
    noise = torch.randn(B, 1, H, D, generator=g, dtype=torch.float64)
    cond = torch.randn(B, 1, OBS_H, OBS_DIM, generator=g, dtype=torch.float64).requires_grad_(True)
    t = torch.randint(0, 1000, (B,), generator=g)
    loss = torch.mean((noise - m(x, t, cond)) ** 2)
    loss.backward()
    out = {"x": x.numpy(), "noise": noise.numpy(), "cond": cond.detach().numpy(), "t": t.numpy(), "wseed": WSEED,
           "weights_sha256": blob_sha256(sd), "loss": loss.item(), "grad_cond": cond.grad.numpy()}
    names = []
    for name, p in m.named_parameters():
        gr = p.grad.detach().reshape(-1).numpy()
        names.append(name)
        out[f"norm/{name}"] = np.linalg.norm(gr)
        out[f"sum/{name}"] = gr.sum()
        out[f"samp/{name}"] = gr[sample_indices(name, gr.size)]
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(names), "tensors, loss", loss.item())


if __name__ == "__main__":
    main()
