"""Training-loss gradients of UNet_Film -- with its six SelfAttention blocks -- on the HIP path (spdm_train_loss_grad on a
SPDM_FLAG_TRAIN | SPDM_FLAG_TRAIN_ATTENTION handle, SpdmEngine(train_attention=True)) against float64 autograd through the
oracle (oracle/unet_film_ref.py, attention=True).

Bound: every tensor's gradient, and d loss / d cond, within ||g - g64||_2 <= 1e-4 ||g64||_2; the loss within 1e-6 relative.
Training is exact fp32 on any handle, so "split" and "exact" differ only in the handle's own state.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle.unet_film_ref import unet_film_forward
from state_policy_diffusionmodel_amd import _lib
from state_policy_diffusionmodel_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

COND_DIM = 14
T_STEPS = 100
BOUND = 1e-4


def _oracle_loss_grad(sd, x, t, cond, noise, dtype=torch.float64):
    params = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in sd.items()}
    c = cond.to(dtype).requires_grad_(True) if cond is not None else None
    fwd = getattr(unet_film_forward, "__wrapped__", unet_film_forward)
    with torch.enable_grad():
        eps = fwd(params, x.to(dtype), t, c, attention=True)
        loss = torch.mean((noise.to(dtype) - eps) ** 2)
        loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in params.items()}
    return loss.detach(), eps.detach(), grads, (c.grad if c is not None else None)


def _data(B, H, D, seed, t_mode):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, H, D, generator=g)
    noise = torch.randn(B, 1, H, D, generator=g)
    cond = torch.randn(B, 1, 2, COND_DIM // 2, generator=g) if t_mode != "nocond" else None
    if t_mode == "broadcast":
        t = torch.randint(0, T_STEPS, (1,), generator=g)
    else:
        t = torch.randint(0, T_STEPS, (B,), generator=g)
    return x, t, cond, noise


def _engine(H, D, B, exact, sd, **kw):
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    eng = SpdmEngine(H, D, COND_DIM, max_batch=B, attention=True, num_train_timesteps=T_STEPS, exact_fp32=exact,
                     train_attention=True, **kw)
    eng.load_state_dict(sd)
    return eng


_REF = {}


def _reference(case, t_mode):
    key = (case, t_mode)
    if key not in _REF:
        B, H, D = case
        sd = random_state_dict(COND_DIM, seed=11, attention=True)
        x, t, cond, noise = _data(B, H, D, 5, t_mode)
        _REF[key] = (sd, x, t, cond, noise, _oracle_loss_grad(sd, x, t, cond, noise))
    return _REF[key]


def _check(got, want, what, worst):
    g = got.detach().double().cpu()
    w = want.double()
    den = float(w.norm())
    err = float((g - w).norm())
    if den == 0.0:
        assert err == 0.0, f"{what}: expected exact zeros, |g| = {err:.3e}"
        return
    worst[what] = err / den


def _assert_within(worst):
    bad = {k: v for k, v in worst.items() if not v <= BOUND}
    assert not bad, "||g - g64|| / ||g64|| above %g: %s" % (BOUND, ", ".join(f"{k} {v:.2e}" for k, v in sorted(bad.items())))


CASES = [(shape, mode) for shape in ((2, 16, 3), (16, 31, 3), (64, 32, 3), (8, 64, 6))
         for mode in ("per_sample", "broadcast", "nocond")]


def _cls(name):
    if name == "grad_cond":
        return "grad_cond"
    if name.endswith(".bias") or name.endswith("in_proj_bias"):
        return "bias"
    if name.startswith("sa") and (".ln." in name or "ff_self.0." in name):
        return "LayerNorm affine"
    if "norm." in name:
        return "GroupNorm affine"
    if ".attention." in name:
        return "attention projection"
    if "ff_self" in name:
        return "ff Linear"
    if "emb_layer" in name or "cond_encoder" in name:
        return "Linear weight"
    return "conv weight"


def _print_classes(tag, worst):
    per = {}
    for k, v in worst.items():
        per[_cls(k)] = max(per.get(_cls(k), 0.0), v)
    print(f"\nCLASSES {tag}: " + ", ".join(f"{c} {v:.2e}" for c, v in sorted(per.items())))


@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("case,t_mode", CASES, ids=[f"B{c[0]}_H{c[1]}_D{c[2]}_{m}" for c, m in CASES])
def test_gradients_match_float64_oracle(case, t_mode, exact):
    B, H, D = case
    sd, x, t, cond, noise, (loss64, eps64, g64, gc64) = _reference(case, t_mode)
    eng = _engine(H, D, B, exact, sd)
    loss, eps, grads, gcond = eng.loss_and_grad(x.cuda(), t, cond.cuda() if cond is not None else None, noise.cuda())
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss64)) <= 1e-6 * float(loss64), (float(loss), float(loss64))
    assert float((eps.cpu().double() - eps64).norm()) <= 1e-5 * float(eps64.norm())
    worst = {}
    assert set(grads) == set(g64)
    assert any(n.startswith("sa6.attention.") for n in grads)
    for name, want in g64.items():
        _check(grads[name], want, name, worst)
    if gc64 is not None:
        _check(gcond.reshape(gc64.shape), gc64, "grad_cond", worst)
    _print_classes(f"{case} {t_mode} {'exact' if exact else 'split'}", worst)
    _assert_within(worst)
    eng.close()


def test_deterministic():
    B, H, D = 8, 16, 3
    sd = random_state_dict(COND_DIM, seed=2, attention=True)
    x, t, cond, noise = _data(B, H, D, 1, "per_sample")
    eng = _engine(H, D, B, False, sd)
    a = eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda(), flat=True)
    b = eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda(), flat=True)
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and float(a[0]) == float(b[0])
    eng.close()


def test_batch_gradient_is_mean_of_samples():
    B, H, D = 4, 16, 3
    sd = random_state_dict(COND_DIM, seed=6, attention=True)
    x, t, cond, noise = _data(B, H, D, 3, "per_sample")
    eng = _engine(H, D, B, True, sd)
    _, _, gB, _ = eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda(), flat=True)
    gB = gB.double().cpu()
    acc = torch.zeros_like(gB)
    for b in range(B):
        _, _, g1, _ = eng.loss_and_grad(x[b:b + 1].cuda(), t[b:b + 1], cond[b:b + 1].cuda(), noise[b:b + 1].cuda(), flat=True)
        acc += g1.double().cpu()
    acc /= B
    for n, off, shape in eng._index:
        cnt = int(np.prod(shape))
        w = acc[off:off + cnt]
        den = float(w.norm())
        if den > 0:
            assert float((gB[off:off + cnt] - w).norm()) <= BOUND * den, n
    eng.close()


@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_forward_and_sampling_match_plain_attention_handle(exact):
    """Every entry point but spdm_train_loss_grad behaves as on a plain attention handle: bit-identical eps and samples."""
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    B, H, D = 8, 32, 3
    sd = random_state_dict(COND_DIM, seed=7, attention=True)
    x, t, cond, _ = _data(B, H, D, 2, "per_sample")
    plain = SpdmEngine(H, D, COND_DIM, max_batch=B, attention=True, num_train_timesteps=T_STEPS, exact_fp32=exact)
    plain.load_state_dict(sd)
    eng = _engine(H, D, B, exact, sd)
    out = []
    for e in (plain, eng):
        eps = e.unet_forward(x.cuda(), t, cond.cuda()).cpu()
        e.set_builtin_schedule(_lib.SPDM_DDIM, T_STEPS, 10)
        g = torch.Generator().manual_seed(3)
        x_T = torch.randn(B, 1, H, D, generator=g)
        smp = e.sample(cond.cuda(), x_T.cuda(), seed=5).cpu()
        out.append((eps, smp))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    plain.close()
    eng.close()


def test_refusals():
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    lib = _lib.load()
    TA, TR = _lib.SPDM_FLAG_TRAIN_ATTENTION, _lib.SPDM_FLAG_TRAIN

    def create(attention, flags, H=16):
        cfg = _lib.SpdmConfig(H, 3, COND_DIM, 256, attention, 2, 0, T_STEPS, flags)
        h = ctypes.c_void_p()
        rc = lib.spdm_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc == 0:
            lib.spdm_destroy(h)
        return rc

    assert create(1, TR) == -1                                # documented: attention needs the new flag
    assert "SPDM_FLAG_TRAIN_ATTENTION" in lib.spdm_last_error().decode()
    assert create(1, TA) == -1                                # the new flag without SPDM_FLAG_TRAIN
    assert create(0, TR | TA) == -1                           # ... with attention = 0
    assert create(0, TR | TA | _lib.SPDM_FLAG_SIMPLE_UNET) == -1
    assert create(1, TR | TA | _lib.SPDM_FLAG_SIMPLE_UNET) == -1
    assert create(1, TR | TA, H=65) == -1                     # sa6 would have 576 tokens
    assert create(1, TR | TA) == 0
    with pytest.raises(ValueError):
        SpdmEngine(16, 3, COND_DIM, max_batch=2, attention=False, train_attention=True)
    with pytest.raises(ValueError):
        SpdmEngine(16, 3, COND_DIM, max_batch=2, model="UNet", num_train_timesteps=1001, train_attention=True)


def _facade_batch(B, T, g):
    return {"position": torch.randn(B, T, 2, generator=g), "action": torch.randn(B, T, 3, generator=g),
            "velocity": torch.randn(B, T, 2, generator=g), "image_features": torch.randn(B, T, 4, generator=g)}


def test_training_step_backward_unet_film_against_oracle():
    """Diffusion_DDPM(model='UNet_Film', train_attention=True).training_step(backward=True): loss, grads() over every named
    parameter and grad_cond against float64 oracle autograd; load_state_dict reaches the cached training engine."""
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    g = torch.Generator().manual_seed(12)
    obs_h, pred_h, inp_h, B = 3, 13, 3, 4
    kw = dict(noise_steps=50, obs_horizon=obs_h, pred_horizon=pred_h, observation_dim=11, prediction_dim=5,
              model="UNet_Film", inpaint_horizon=inp_h)
    m = Diffusion_DDPM(**kw, weight_seed=3, max_batch=B, train_attention=True)
    batch = _facade_batch(B, obs_h + pred_h, g)
    t = torch.tensor([0, 9, 23, 49])
    noise = torch.randn(B, 1, pred_h + inp_h, 5, generator=g)
    loss, eps, x_noisy = m.training_step({k: v.clone() for k, v in batch.items()}, t=t, noise=noise, return_parts=True,
                                         backward=True)
    obs = {k: v[:, :obs_h].float() for k, v in batch.items()}
    cond = torch.cat([obs["position"], obs["action"], obs["velocity"], obs["image_features"]], -1).unsqueeze(1)
    loss64, _, g64, gc64 = _oracle_loss_grad(m.noise_estimator._sd, x_noisy.cpu(), t, cond, noise)
    assert abs(float(loss) - float(loss64)) <= 1e-6 * float(loss64)
    worst = {}
    grads = m.noise_estimator.grads()
    assert set(grads) == set(g64) == set(m.noise_estimator._sd)
    for name, want in g64.items():
        _check(grads[name], want, name, worst)
    _check(m.noise_estimator.grad_cond.reshape(gc64.shape), gc64, "grad_cond", worst)
    _print_classes("training_step", worst)
    _assert_within(worst)
    sd2 = {k: v * 0.5 for k, v in m.noise_estimator._sd.items()}
    m.noise_estimator.load_state_dict(sd2)
    loss2, eps2, _ = m.training_step({k: v.clone() for k, v in batch.items()}, t=t, noise=noise, return_parts=True,
                                     backward=True)
    want2 = unet_film_forward(sd2, x_noisy.cpu(), t, cond, attention=True)
    assert float((eps2.cpu() - want2).abs().max()) <= 1e-4
    assert abs(float(loss2) - float(torch.mean((noise - want2) ** 2))) <= 1e-5
    with pytest.raises(NotImplementedError, match="train_attention"):
        Diffusion_DDPM(**kw).training_step(batch, t=t, noise=noise, backward=True)


def test_short_adam_run_tracks_fp32_oracle():
    """20 torch-Adam steps (lr 1e-3, fixed data) on the HIP gradients and on fp32 oracle autograd from the same start."""
    B, H, D = 8, 16, 3
    sd0 = random_state_dict(COND_DIM, seed=8, attention=True)
    x, t, cond, noise = _data(B, H, D, 4, "per_sample")
    names = list(sd0)
    flat0 = torch.cat([torch.as_tensor(np.asarray(sd0[n])).reshape(-1) for n in names])
    shapes = [np.asarray(sd0[n]).shape for n in names]

    def unflat(v):
        out, off = {}, 0
        for n, s in zip(names, shapes):
            k = int(np.prod(s)) if s else 1
            out[n] = v[off:off + k].reshape(s).numpy()
            off += k
        return out

    eng = _engine(H, D, B, True, sd0)
    p_hip = flat0.clone().cuda().requires_grad_(True)
    p_ref = flat0.clone().requires_grad_(True)
    opt_hip = torch.optim.Adam([p_hip], lr=1e-3)
    opt_ref = torch.optim.Adam([p_ref], lr=1e-3)
    losses = []
    for step in range(20):
        if step:
            eng.load_state_dict(unflat(p_hip.detach().cpu()))
        loss, _, g, _ = eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda(), flat=True)
        p_hip.grad = g.clone()
        opt_hip.step()
        lr, _, gr, _ = _oracle_loss_grad(unflat(p_ref.detach()), x, t, cond, noise, torch.float32)
        p_ref.grad = torch.cat([gr[n].reshape(-1) for n in names])
        opt_ref.step()
        lh, lr_ = float(loss), float(lr)
        assert abs(lh - lr_) <= 1e-3 * lr_, (step, lh, lr_)
        losses.append(lh)
    assert losses[-1] < losses[0]
    eng.close()
