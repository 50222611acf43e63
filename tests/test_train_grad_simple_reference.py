"""Pin of the oracle's BACKWARD pass through simple_Unet.py's UNet against the reference module: float64 autograd through
tests/simple_unet_ref.py must reproduce the gradients that ``tools/make_golden_train.py --simple`` recorded from the imported
reference UNet (tests/golden/train_grad_simple_h16d3_b2.npz: B = 2, H = 16, D = 3, per-sample t, float64), in eval mode and
with PositionalEncoding's dropout replaced by a fixed mask multiply.  The dropout case goes through the oracle unchanged: its
table is pe[t] * scale and its timesteps arange(B).  The GPU gradient tests (test_gpu_train_grad_simple.py) compare against
the same oracle autograd.  No GPU, no reference import."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from simple_unet_ref import simple_unet_forward
from state_policy_diffusionmodel_amd.weights import blob_sha256, random_state_dict

N_SAMPLES = 256
REL = 1e-9          # both sides float64: the differences are summation order only
PE = "pos_encoding.pos_encoding"


def sample_indices(name: str, numel: int) -> np.ndarray:
    seed = int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little") ^ numel
    return np.random.default_rng(seed).integers(0, numel, N_SAMPLES)


def _autograd(g, sd, prefix):
    params = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items()}
    t = torch.from_numpy(g["t"])
    if prefix == "drop/":
        params[PE] = params[PE][t] * torch.from_numpy(g["drop/scale"])
        t = torch.arange(t.numel())
    for k, p in params.items():
        if k != PE:
            p.requires_grad_(True)
    c = torch.from_numpy(g["cond"]).clone().requires_grad_(True)
    fwd = getattr(simple_unet_forward, "__wrapped__", simple_unet_forward)
    with torch.enable_grad():
        eps = fwd(params, torch.from_numpy(g["x"]), t, c)
        loss = torch.mean((torch.from_numpy(g["noise"]) - eps) ** 2)
        loss.backward()
    return {k: p for k, p in params.items() if k != PE}, c, loss


@pytest.fixture(scope="module")
def pinned():
    g = np.load(os.path.join(GOLDEN, "train_grad_simple_h16d3_b2.npz"))
    cond_dim = g["cond"].shape[-2] * g["cond"].shape[-1]
    sd = random_state_dict(cond_dim, seed=int(g["wseed"]), model="UNet", noise_steps=int(g["noise_steps"]))
    assert blob_sha256(sd) == str(g["weights_sha256"]), "weight generator drifted from the fixture"
    return g, {prefix: _autograd(g, sd, prefix) for prefix in ("", "drop/")}


@pytest.mark.parametrize("prefix", ["", "drop/"], ids=["eval", "dropout_mask"])
def test_fixture_covers_every_parameter(pinned, prefix):
    g, runs = pinned
    params, _, _ = runs[prefix]
    names = sorted(str(n) for n in g[prefix + "names"])
    assert names == sorted(params)
    assert PE not in names                                     # a buffer: no gradient
    for blk in ("down1", "down2", "down3", "up1", "up2", "up3"):
        assert f"{blk}.cond_emb_layer.1.weight" in names and f"{blk}.doubleConv1.norm.bias" in names


@pytest.mark.parametrize("prefix", ["", "drop/"], ids=["eval", "dropout_mask"])
def test_loss_and_grad_cond_match_reference(pinned, prefix):
    g, runs = pinned
    _, c, loss = runs[prefix]
    assert abs(loss.item() - float(g[prefix + "loss"])) <= REL * float(g[prefix + "loss"])
    want = g[prefix + "grad_cond"]
    assert np.linalg.norm(c.grad.numpy() - want) <= REL * np.linalg.norm(want)


@pytest.mark.parametrize("prefix", ["", "drop/"], ids=["eval", "dropout_mask"])
def test_parameter_gradients_match_reference(pinned, prefix):
    g, runs = pinned
    params, _, _ = runs[prefix]
    bad = []
    for name, p in params.items():
        got = p.grad.reshape(-1).numpy()
        norm = float(g[f"{prefix}norm/{name}"])
        ok = abs(np.linalg.norm(got) - norm) <= REL * norm
        ok &= abs(got.sum() - float(g[f"{prefix}sum/{name}"])) <= REL * norm * np.sqrt(got.size)
        ok &= np.abs(got[sample_indices(name, got.size)] - g[f"{prefix}samp/{name}"]).max() <= REL * norm
        if not ok:
            bad.append(name)
    assert not bad, f"oracle gradients differ from the reference's: {bad}"


def test_dropout_moves_the_time_path(pinned):
    """The mask is not a no-op: the emb_layer gradients of the two cases differ by far more than REL, while the fixture's
    mask keeps about 90 % of the entries."""
    g, _ = pinned
    scale = g["drop/scale"]
    assert 0.8 < float((scale > 0).mean()) < 0.97
    for blk in ("down1", "up3"):
        a, b = float(g[f"norm/{blk}.emb_layer.1.weight"]), float(g[f"drop/norm/{blk}.emb_layer.1.weight"])
        assert abs(a - b) > 1e3 * REL * a
