"""The concat-conditioned U-Net of the reference's models/simple_Unet.py (``Diffusion_DDPM``'s default ``model='UNet'``),
CPU side: the parameter spec against the reference module's recorded inventory, the torch-CPU restatement
(tests/simple_unet_ref.py) against the fixtures recorded from the reference module (tools/make_golden_simple.py), and the
facade's construction / checkpoint paths.  The device path is tests/test_gpu_simple_unet.py."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN
from oracle.scheduler_ref import sample_loop
from simple_unet_ref import simple_unet_forward
from state_policy_diffusionmodel_amd import weights
from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDIM, Diffusion_DDPM, load_model

EPS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "simple_unet_*.npz")))
TRAJ_FILES = sorted(glob.glob(os.path.join(GOLDEN, "simple_traj_*.npz")))


def _weights(g):
    cond_dim = int(g["obs_h"]) * int(g["obs_dim"])
    sd = weights.random_state_dict(cond_dim, seed=int(g["wseed"]), model="UNet", noise_steps=int(g["noise_steps"]))
    assert weights.blob_sha256(sd) == str(g["weights_sha256"]), "weight generator drifted from the fixtures"
    return sd


@pytest.mark.parametrize("cond_dim", [20, 1350])
def test_param_spec_is_the_reference_inventory(cond_dim):
    inv = json.load(open(os.path.join(GOLDEN, "simple_inventory.json")))[f"cond_dim_{cond_dim}"]
    spec = weights.unet_simple_param_spec(cond_dim, noise_steps=1000)
    assert [[k, list(v)] for k, v in spec.items()] == inv
    assert len(spec) == 79


def test_pos_encoding_buffer_is_interleaved_sin_cos():
    pe = weights.simple_pos_encoding(1001, 256)
    assert pe.shape == (1001, 256)
    p, i = 37, 5
    w = np.exp(-np.log(10000.0) * 2 * i / 256)
    assert abs(pe[p, 2 * i] - np.sin(p * w)) < 1e-5 and abs(pe[p, 2 * i + 1] - np.cos(p * w)) < 1e-5


@pytest.mark.parametrize("path", EPS_FILES, ids=[os.path.basename(p) for p in EPS_FILES])
def test_restatement_reproduces_reference_eps(path):
    g = np.load(path)
    sd = _weights(g)
    assert len(EPS_FILES) == 5
    for i in range(2):
        got = simple_unet_forward(sd, torch.from_numpy(g["x"]), torch.from_numpy(g[f"t{i}"]), torch.from_numpy(g["cond"]))
        assert np.abs(got.numpy() - g[f"eps{i}"]).max() <= 2e-5


@pytest.mark.parametrize("path", TRAJ_FILES, ids=[os.path.basename(p) for p in TRAJ_FILES])
def test_restatement_reproduces_reference_trajectory(path):
    g = np.load(path)
    sd = _weights(g)
    inpaint = torch.from_numpy(g["inpaint"]) if "inpaint" in g.files else None
    hist = sample_loop(lambda x, t, y: simple_unet_forward(sd, x, t, y), str(g["kind"]), int(g["T"]), int(g["N"]),
                       torch.from_numpy(g["cond"]), torch.from_numpy(g["x_T"]),
                       torch.from_numpy(g["noise"]) if str(g["kind"]) == "ddpm" else None, inpaint, history=True)
    assert np.abs(np.stack([h.numpy() for h in hist]) - g["history"]).max() <= 1e-4


def test_restatement_needs_conditioning():
    sd = weights.random_state_dict(20, model="UNet", noise_steps=10)
    with pytest.raises(ValueError):
        simple_unet_forward(sd, torch.zeros(1, 1, 8, 2), torch.tensor([1]), None)


def test_reference_default_arguments_construct_the_simple_network():
    m = Diffusion_DDPM()
    assert m.simple and not m.attention and m.model_name == "UNet"
    sd = m.noise_estimator.state_dict()
    assert list(sd) == list(weights.unet_simple_param_spec(20, noise_steps=1000))
    assert tuple(sd["pos_encoding.pos_encoding"].shape) == (1001, 256)
    # any non-FiLM name builds the same network (models/diffusion_ddpm.py:53-62)
    assert Diffusion_DDIM(model="something_else", noise_steps=50).simple


def _write_ckpt(tmp_path, hp, sd):
    full = {"noise_estimator." + k: torch.from_numpy(np.array(v)) for k, v in weights.state_dict_to_numpy(sd).items()}
    cp, yp = tmp_path / "epoch=1.ckpt", tmp_path / "hparams.yaml"
    torch.save({"state_dict": full, "hyper_parameters": dict(hp)}, cp)
    yp.write_text(yaml.safe_dump(hp))
    return str(cp), str(yp)


@pytest.mark.parametrize("with_model_key", [True, False])
def test_load_from_checkpoint_builds_the_simple_network(tmp_path, with_model_key):
    hp = dict(noise_steps=100, obs_horizon=3, pred_horizon=8, observation_dim=5, prediction_dim=2, inpaint_horizon=2)
    if with_model_key:
        hp["model"] = "UNet"
    sd = weights.random_state_dict(15, seed=4, model="UNet", noise_steps=100)
    cp, yp = _write_ckpt(tmp_path, hp, sd)
    m = Diffusion_DDPM.load_from_checkpoint(cp, hparams_file=yp)
    assert m.simple and m.cond_dim == 15
    got = m.noise_estimator.state_dict()
    assert list(got) == list(sd) and all(np.array_equal(got[k].numpy(), sd[k]) for k in sd)
    d = load_model("DDIM", cp, yp, 20)
    assert isinstance(d, Diffusion_DDIM) and d.simple and d.noise_steps == 20


def test_mismatched_state_dicts_are_rejected(tmp_path):
    film = weights.random_state_dict(15, seed=1, attention=False)
    simple = weights.random_state_dict(15, seed=1, model="UNet", noise_steps=100)
    with pytest.raises(ValueError, match="UNet_Film"):
        weights.check_state_dict(film, 15, model="UNet", noise_steps=100)
    with pytest.raises(ValueError, match="model='UNet'"):
        weights.check_state_dict(simple, 15, attention=False, model="UNet_FilmnoAttention")
    with pytest.raises(ValueError, match="shape"):
        weights.check_state_dict(simple, 15, model="UNet", noise_steps=200)      # pos_encoding rows = noise_steps + 1
    hp = dict(noise_steps=100, obs_horizon=3, observation_dim=5, model="UNet")
    cp, yp = _write_ckpt(tmp_path, hp, film)
    with pytest.raises(ValueError, match="UNet_Film"):
        Diffusion_DDPM.load_from_checkpoint(cp, hparams_file=yp)
    cp, yp = _write_ckpt(tmp_path, dict(hp, model="UNet_Film"), simple)
    with pytest.raises(ValueError, match="model='UNet'"):
        Diffusion_DDPM.load_from_checkpoint(cp, hparams_file=yp)
