"""GPU tests (pytest -m gpu) of the concat-conditioned U-Net (the reference's models/simple_Unet.py, ``model='UNet'``) on
libspdm_hip.so (SPDM_FLAG_SIMPLE_UNET): eps and trajectories against the fixtures recorded from the reference module
(tools/make_golden_simple.py), large batches against the CPU restatement (tests/simple_unet_ref.py), batch independence,
graph replay, the facade and the error paths.  Tolerance 1e-4 absolute, the FiLM networks' bar."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.scheduler_ref import sample_loop
from simple_unet_ref import simple_unet_forward
from state_policy_diffusionmodel_amd.weights import blob_sha256, random_state_dict

pytestmark = pytest.mark.gpu
TOL = 1e-4
EPS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "simple_unet_*.npz")))
TRAJ_FILES = sorted(glob.glob(os.path.join(GOLDEN, "simple_traj_*.npz")))
_SD = {}


def weights(cond_dim, seed=0, noise_steps=1000, sha=None):
    key = (cond_dim, seed, noise_steps)
    if key not in _SD:
        _SD[key] = random_state_dict(cond_dim, seed=seed, model="UNet", noise_steps=noise_steps)
    if sha is not None:
        assert blob_sha256(_SD[key]) == sha, "weight generator drifted from the fixtures"
    return _SD[key]


def make_engine(H, D, cond_dim, B, sd, exact_fp32=False):
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    eng = SpdmEngine(H, D, cond_dim, max_batch=B, model="UNet", exact_fp32=exact_fp32,
                     num_train_timesteps=sd["pos_encoding.pos_encoding"].shape[0])
    eng.load_state_dict(sd)
    return eng


@pytest.mark.parametrize("exact", [False, True], ids=["split_fp16", "exact_fp32"])
@pytest.mark.parametrize("path", EPS_FILES, ids=[os.path.basename(p) for p in EPS_FILES])
def test_eps_matches_reference_fixture(path, exact):
    g = np.load(path)
    H, D, B = int(g["H"]), int(g["D"]), int(g["B"])
    cond_dim = int(g["obs_h"]) * int(g["obs_dim"])
    sd = weights(cond_dim, int(g["wseed"]), int(g["noise_steps"]), str(g["weights_sha256"]))
    eng = make_engine(H, D, cond_dim, B, sd, exact_fp32=exact)
    assert eng.split_precision == (not exact)
    x, cond = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["cond"]).cuda()
    try:
        for i in range(2):                     # scalar t, then one t per sample
            got = eng.unet_forward(x, g[f"t{i}"], cond).cpu().numpy()
            err = float(np.abs(got - g[f"eps{i}"]).max())
            print(f"{os.path.basename(path)} t{i} {'exact' if exact else 'split'}: max |eps - ref| = {err:.2e}")
            assert got.shape == g[f"eps{i}"].shape and err <= TOL, (path, i, err)
    finally:
        eng.close()


@pytest.mark.parametrize("path", TRAJ_FILES, ids=[os.path.basename(p) for p in TRAJ_FILES])
def test_trajectory_matches_reference_fixture(path):
    from state_policy_diffusionmodel_amd.schedulers import DDIMScheduler, DDPMScheduler
    g = np.load(path)
    H, D, B, T, N = (int(g[k]) for k in ("H", "D", "B", "T", "N"))
    cond_dim = int(g["obs_h"]) * int(g["obs_dim"])
    sd = weights(cond_dim, int(g["wseed"]), int(g["noise_steps"]), str(g["weights_sha256"]))
    eng = make_engine(H, D, cond_dim, B, sd)
    sched = (DDPMScheduler if str(g["kind"]) == "ddpm" else DDIMScheduler)(num_train_timesteps=T)
    sched.set_timesteps(N)
    eng.set_scheduler(sched)
    inpaint = torch.from_numpy(g["inpaint"]).cuda() if "inpaint" in g.files else None
    noise = torch.from_numpy(g["noise"]).cuda() if str(g["kind"]) == "ddpm" else None
    try:
        _, hist = eng.sample(torch.from_numpy(g["cond"]).cuda(), torch.from_numpy(g["x_T"]).cuda(), noise=noise,
                             inpaint=inpaint, history=True)
        err = float(np.abs(hist.cpu().numpy() - g["history"]).max())
        print(f"{os.path.basename(path)}: max |iterate - ref| over {N + 1} iterates = {err:.2e}")
        assert err <= TOL
    finally:
        eng.close()


def _inputs(B, H=32, D=3, n=3, seed=2024, rows_total=4096):
    """cond, x_T, noise for B trajectories; row b gets the same values whatever B is (drawn for rows_total rows, sliced)"""
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(rows_total, 1, 10, 2, generator=g)[:B].contiguous()
    x_T = torch.rand(rows_total, 1, H, D, generator=g)[:B].contiguous()
    noise = torch.randn(n, rows_total, 1, H, D, generator=g)[:, :B].contiguous()
    return cond, x_T, noise


def _device_loop(B, cond, x_T, noise, H=32, D=3, switch=None):
    """a three-step DDPM loop (T = 3: timesteps 2, 1, 0) with pre-drawn noise on the device"""
    from state_policy_diffusionmodel_amd.schedulers import DDPMScheduler
    eng = make_engine(H, D, 20, B, weights(20))
    if switch:
        eng.set_switch(switch, True)
    sched = DDPMScheduler(num_train_timesteps=3)
    sched.set_timesteps(3)
    eng.set_scheduler(sched)
    try:
        out, hist = eng.sample(cond.cuda(), x_T.cuda(), noise=noise.cuda(), history=True)
        return out.cpu(), hist.cpu()
    finally:
        eng.close()


@pytest.mark.parametrize("B", [256, 4096])
def test_large_batch_matches_restatement(B):
    cond, x_T, noise = _inputs(B)
    got, _ = _device_loop(B, cond, x_T, noise)
    rows = list(range(B)) if B <= 256 else sorted(set(range(0, B, 64)) | {B - 1})
    sd = weights(20)
    want = sample_loop(lambda x, t, y: simple_unet_forward(sd, x, t, y), "ddpm", 3, 3, cond[rows], x_T[rows],
                       noise[:, rows], None)
    err = float((got[rows] - want).abs().max())
    print(f"B={B}: max |x_0 - restatement| over {len(rows)} rows = {err:.2e}")
    assert err <= TOL


def test_batch_independence():
    outs = {B: _device_loop(B, *_inputs(B))[0] for B in (1, 64, 4096)}
    for B in (64, 4096):
        d = float((outs[B][:1] - outs[1]).abs().max())
        print(f"row 0 of B={B} vs B=1: {d:.2e}")
        assert d <= 2e-6
    d = float((outs[4096][:64] - outs[64]).abs().max())
    print(f"rows 0..63 of B=4096 vs B=64: {d:.2e}")
    assert d <= 2e-6


def test_graph_replay_is_bit_identical_to_plain_launches():
    cond, x_T, noise = _inputs(8)
    a, ha = _device_loop(8, cond, x_T, noise)
    b, hb = _device_loop(8, cond, x_T, noise, switch="SPDM_NO_GRAPH")
    assert torch.equal(a, b) and torch.equal(ha, hb)


def _obs_batch(m, B, g):
    return {"obs_cond": torch.randn(B, m.obs_horizon, m.observation_dim, generator=g),
            "inpaint": torch.rand(B, m.inpaint_horizon, m.prediction_dim, generator=g)}


def test_facade_reference_defaults_sample():
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    m = Diffusion_DDPM()                                     # model='UNet', noise_steps=1000, H = 10 + 10, D = 2
    g = torch.Generator().manual_seed(0)
    x = m.sample(_obs_batch(m, 3, g), seed=1)
    assert tuple(x.shape) == (1, 1, 20, 2) and bool(torch.isfinite(x).all())
    assert m._engine.graph_captures == 1
    x2 = m.sample(_obs_batch(m, 3, g), seed=2)               # fresh tensors: the captured step is replayed
    assert tuple(x2.shape) == (1, 1, 20, 2) and m._engine.graph_captures == 1
    hist = m.sample(_obs_batch(m, 1, g), option="sample_history", seed=3)
    assert len(hist) == 1001 and all(tuple(h.shape) == (1, 1, 20, 2) for h in hist)


def test_facade_matches_restatement_and_ddim_swap():
    from state_policy_diffusionmodel_amd.diffusion import load_model
    from state_policy_diffusionmodel_amd.schedulers import DDIMScheduler
    m = load_model("DDIM", None, None, 10, noise_steps=100, obs_horizon=2, pred_horizon=6, observation_dim=3,
                   prediction_dim=2, inpaint_horizon=2, model="UNet", weight_seed=6)
    assert isinstance(m.noise_scheduler, DDIMScheduler) and m.simple
    g = torch.Generator().manual_seed(5)
    obs = _obs_batch(m, 4, g)
    x_T = torch.rand(4, 1, 8, 2, generator=g)
    got = m.sample(dict(obs), x_T=x_T.cuda(), batched=True).cpu()
    sd = {k: v for k, v in m.noise_estimator.state_dict().items()}
    want = sample_loop(lambda x, t, y: simple_unet_forward(sd, x, t, y), "ddim", 10, 10, obs["obs_cond"].unsqueeze(1),
                       x_T, None, obs["inpaint"].unsqueeze(1))
    assert float((got - want).abs().max()) <= TOL
    # forward half of training_step: per-sample t through spdm_unet_forward
    batch = {"obs_cond": torch.randn(3, 2, 3, generator=g), "inpaint": torch.rand(3, 2, 2, generator=g)}
    eps = m.noise_estimator(torch.rand(3, 1, 8, 2).cuda(), torch.tensor([0, 50, 100]), batch["obs_cond"].unsqueeze(1).cuda())
    assert tuple(eps.shape) == (3, 1, 8, 2)


def test_errors_before_any_launch():
    from state_policy_diffusionmodel_amd import _lib
    sd = weights(20)
    eng = make_engine(16, 3, 20, 2, sd)
    try:
        x = torch.rand(2, 1, 16, 3).cuda()
        cond = torch.randn(2, 20).cuda()
        with pytest.raises(RuntimeError, match="d_cond"):
            eng.unet_forward(x, [5], None)
        with pytest.raises(RuntimeError, match="outside"):
            eng.unet_forward(x, [1001], cond)                 # pos_encoding has noise_steps + 1 = 1001 rows
        eng.set_builtin_schedule(0, 20, 20)
        with pytest.raises(RuntimeError, match="d_cond"):
            eng.sample(None, x)
        assert bool(torch.isfinite(eng.unet_forward(x, [1000], cond)).all())    # the last row is valid
        with pytest.raises(RuntimeError):
            eng.debug_tensor("x1")                           # no SPDM_FLAG_DEBUG_KEEP: an error, not a fault
    finally:
        eng.close()
    lib = _lib.load()
    h = ctypes.c_void_p()
    cfg = _lib.SpdmConfig(16, 3, 20, 256, 1, 2, 0, 1001, _lib.SPDM_FLAG_SIMPLE_UNET)      # attention = 1
    assert lib.spdm_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    bad = SpdmEngine(16, 3, 20, max_batch=1, model="UNet", num_train_timesteps=1000)     # table must have 1001 rows
    try:
        with pytest.raises(RuntimeError, match="pos_encoding"):
            bad.load_state_dict(sd)
    finally:
        bad.close()
    film = random_state_dict(20, seed=0, attention=False)
    other = SpdmEngine(16, 3, 20, max_batch=1, model="UNet", num_train_timesteps=1001)
    try:
        with pytest.raises(KeyError):
            other.load_state_dict(film)
    finally:
        other.close()


def test_debug_taps_and_profiler():
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    sd = weights(20)
    eng = SpdmEngine(32, 3, 20, max_batch=2, model="UNet", num_train_timesteps=1001, debug=True)
    eng.load_state_dict(sd)
    try:
        g = torch.Generator().manual_seed(9)
        x, cond = torch.rand(2, 1, 32, 3, generator=g), torch.randn(2, 1, 10, 2, generator=g)
        eng.unet_forward(x.cuda(), [300], cond.cuda())
        u3 = eng.debug_tensor("u3").cpu()
        assert tuple(u3.shape) == (2, 64, 32, 8)
        x4 = eng.debug_tensor("x4").cpu()
        assert tuple(x4.shape) == (2, 320, 4, 1) and float(x4[:, 288:].abs().max()) == 0.0   # storage padding stays zero
    finally:
        eng.close()
    eng = make_engine(32, 3, 20, 4, sd)
    try:
        eng.set_builtin_schedule(0, 10, 10)
        eng.profile(True)
        eng.sample(torch.randn(4, 20).cuda(), torch.rand(4, 1, 32, 3).cuda())
        n, ms, fl = eng.profile_read()
        assert n > 0 and ms > 0 and fl > 0
        eng.profile(False)
    finally:
        eng.close()
