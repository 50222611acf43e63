"""Training with the timesteps on the device (spdm_train_loss_grad_dt) and training_step(device_noise=True):
bit-identical to the host-t entry and to the torch forward process on the same values, and without a synchronising torch
operation on a side stream.  H = 16, D = 3, cond_dim = 14 as tests/test_gpu_train_grad.py; UNet_FilmnoAttention, UNet_Film with
train_attention and simple_Unet.py's UNet."""
import numpy as np
import pytest
import torch

from forward_process_ref import draw_t, draw_time_scale
from state_policy_diffusionmodel_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

COND_DIM = 14
NOISE_STEPS = 100
H, D = 16, 3
MODELS = ["UNet_FilmnoAttention", "UNet_Film", "UNet"]


def _engine(model, B):
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    if model == "UNet":
        sd = random_state_dict(COND_DIM, seed=11, model="UNet", noise_steps=NOISE_STEPS)
        eng = SpdmEngine(H, D, COND_DIM, max_batch=B, model="UNet", num_train_timesteps=NOISE_STEPS + 1, train_simple=True)
    elif model == "UNet_Film":
        sd = random_state_dict(COND_DIM, seed=11, attention=True)
        eng = SpdmEngine(H, D, COND_DIM, max_batch=B, attention=True, num_train_timesteps=NOISE_STEPS, train_attention=True)
    else:
        sd = random_state_dict(COND_DIM, seed=11, attention=False)
        eng = SpdmEngine(H, D, COND_DIM, max_batch=B, attention=False, num_train_timesteps=NOISE_STEPS, train=True)
    eng.load_state_dict(sd)
    return eng


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("model", MODELS)
def test_device_t_equals_host_t_bit_for_bit(model, B):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 1, H, D, generator=g).cuda()
    noise = torch.randn(B, 1, H, D, generator=g).cuda()
    cond = torch.randn(B, 1, 2, COND_DIM // 2, generator=g).cuda()
    eng = _engine(model, B)
    for t in (torch.randint(0, NOISE_STEPS, (B,), generator=g), torch.randint(0, NOISE_STEPS, (1,), generator=g)):
        want = eng.loss_and_grad(x, t, cond, noise, flat=True)                       # host t (int64 on the CPU)
        got = eng.loss_and_grad(x, t.to(torch.int32).cuda(), cond, noise, flat=True)    # device int32 t: no .cpu()
        torch.cuda.synchronize()
        for name, a, b in zip(("loss", "eps", "grad", "grad_cond"), got, want):
            assert _same(a, b), (name, t.numel())
        assert float(want[2].abs().max()) > 0.0
    # an out-of-range device t is clamped into the table (the host entry rejects it)
    hi = torch.full((B,), NOISE_STEPS + 50, dtype=torch.int32).cuda()
    got = eng.loss_and_grad(x, hi, cond, noise, flat=True)
    want = eng.loss_and_grad(x, torch.full((B,), eng.num_train_timesteps - 1), cond, noise, flat=True)
    torch.cuda.synchronize()
    assert _same(got[0], want[0]) and _same(got[2], want[2])
    with pytest.raises(RuntimeError, match="outside"):
        eng.loss_and_grad(x, hi.cpu(), cond, noise, flat=True)
    eng.close()


# ---- the facade ------------------------------------------------------------------------------------------------------------
OBS_H, PRED_H, INP_H = 2, 14, 2          # H = 16; observation_dim 7 x obs_horizon 2 = cond_dim 14


def _model(model, B):
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    return Diffusion_DDPM(noise_steps=50, obs_horizon=OBS_H, pred_horizon=PRED_H, observation_dim=7, prediction_dim=D, model=model,
                          inpaint_horizon=INP_H, max_batch=B, weight_seed=3, learning_rate=1e-3,
                          train_attention=model == "UNet_Film")


def _batch(B, gen, device="cpu"):
    T = OBS_H + PRED_H
    return {"position": torch.randn(B, T, 2, generator=gen).to(device), "action": torch.randn(B, T, 1, generator=gen).to(device),
            "velocity": torch.randn(B, T, 2, generator=gen).to(device),
            "image_features": torch.randn(B, T, 2, generator=gen).to(device)}


def _clean_window(m, batch):
    obs = m.prepare_observation_batch(batch)
    x_0 = m.prepare_prediction_vectors(m.prepare_prediction_batch(batch)).unsqueeze(1)
    inp = m.prepare_inpaint_vectors(obs).unsqueeze(1)
    return torch.cat([inp, x_0], dim=2), inp


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("model", MODELS)
def test_training_step_device_noise_equals_given_values(model, B):
    m = _model(model, B)
    batch = _batch(B, torch.Generator().manual_seed(4))
    clone = lambda: {k: v.clone() for k, v in batch.items()}  # noqa: E731
    window, inp = _clean_window(m, clone())
    _, noise_dev, t_dev = m.forward_process(window, inp, seed=7, step=3)
    assert np.array_equal(t_dev.cpu().numpy(), draw_t(7, 3, 0, B, 50))

    def parts(**kw):
        out = m.training_step(clone(), backward=True, return_parts=True, **kw)
        grads = {k: v.clone() for k, v in m.noise_estimator.grads().items()}
        return tuple(o.clone() for o in out), grads, m.noise_estimator.grad_cond.clone()

    got = parts(device_noise=True, seed=7, noise_step=3)
    want = parts(t=t_dev, noise=noise_dev)
    torch.cuda.synchronize()
    for name, a, b in zip(("loss", "eps", "x_noisy"), got[0], want[0]):
        assert _same(a, b), name
    assert set(got[1]) == set(want[1]) and len(got[1]) > 10
    for k in got[1]:
        assert _same(got[1][k], want[1][k]), k
    assert _same(got[2], want[2])
    # the internal counter: two calls without noise_step draw steps 0 and 1 of the seed
    x_a = m.training_step(clone(), backward=True, return_parts=True, device_noise=True, seed=7)[2]
    x_b = m.training_step(clone(), backward=True, return_parts=True, device_noise=True, seed=7)[2]
    for step, x in ((0, x_a), (1, x_b)):
        assert _same(x, m.forward_process(window, inp, seed=7, step=step)[0]), step
    if model != "UNet":
        with pytest.raises(ValueError):
            m.training_step(clone(), backward=True, device_noise=True, time_dropout=0.1)
        return
    # simple_Unet.py: the dropout mask drawn in the same launch against the same mask passed as time_scale
    mask = m.forward_process(window, inp, seed=7, step=3, time_dim=256, dropout_p=0.1)[3]
    assert np.array_equal(mask.cpu().numpy(), draw_time_scale(7, 3, 0, B, 256, 0.1))
    got = parts(device_noise=True, seed=7, noise_step=3, time_dropout=0.1)
    want_d = parts(t=t_dev, noise=noise_dev, time_scale=mask)
    torch.cuda.synchronize()
    for name, a, b in zip(("loss", "eps", "x_noisy"), got[0], want_d[0]):
        assert _same(a, b), name
    for k in got[1]:
        assert _same(got[1][k], want_d[1][k]), k
    assert _same(got[2], want_d[2])
    assert not _same(got[0][1], want[0][1])                  # and the mask does reach the network
    with pytest.raises(ValueError):
        m.training_step(clone(), backward=True, device_noise=True, time_dropout=0.1, time_scale=mask)


def test_side_stream_step_runs_no_synchronising_torch_operation():
    """On a side stream a device_noise step + optimizer_step(DeviceAdam) runs no synchronising torch operation: no .cpu() of t,
    no host-side draw.  The debug mode sees torch's own operations only; the waits inside the library (DESIGN.md 8.9 lists
    them) remain and are not what this checks."""
    B = 2
    m = _model("UNet_FilmnoAttention", B)
    opt = m.configure_optimizers(device_optimizer=True)["optimizer"]
    batch = _batch(B, torch.Generator().manual_seed(4), device="cuda")       # a host batch would synchronise in its upload
    m.training_step(dict(batch), backward=True, device_noise=True, seed=1)   # builds the engine (that does synchronise)
    m.optimizer_step(opt, 0.5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").item()
            probe = False
        except RuntimeError:
            probe = True
        if not probe:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this torch build: nothing to observe")
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                loss = m.training_step(dict(batch), backward=True, device_noise=True, seed=1)
                m.optimizer_step(opt, 0.5)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    side.synchronize()
    assert np.isfinite(float(loss)) and opt.state[opt.param_groups[0]["params"][0]]["step"] == 3
