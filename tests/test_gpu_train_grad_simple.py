"""Training-loss gradients of the reference's default network -- models/simple_Unet.py's concat-conditioned UNet -- on the HIP
path (spdm_train_loss_grad on a SPDM_FLAG_TRAIN | SPDM_FLAG_SIMPLE_UNET | SPDM_FLAG_TRAIN_SIMPLE handle,
SpdmEngine(model='UNet', train_simple=True)) against float64 autograd through the CPU restatement (tests/simple_unet_ref.py),
in eval mode and with PositionalEncoding's dropout as a per-sample multiplier of pe[t] (spdm_train_set_time_scale).

Bound: every parameter's gradient, and d loss / d cond, within ||g - g64||_2 <= 1e-4 ||g64||_2; the loss within 1e-6 relative.
Training is exact fp32 on any handle, so "split" and "exact" differ only in the handle's own state.
Measured worst ratios per tensor class over every case below (MI355X): conv weight 5.1e-6, GroupNorm affine 6.6e-6,
emb_layer 4.3e-6, cond_emb_layer 5.3e-6, outc 1.5e-6, bias 4.5e-6, grad_cond 3.4e-6 (all from the edge-data case; the
largest batch, B = 256, stays below 1.3e-6).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from simple_unet_ref import simple_unet_forward
from state_policy_diffusionmodel_amd import _lib
from state_policy_diffusionmodel_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

COND_DIM = 14
NOISE_STEPS = 100
T_ROWS = NOISE_STEPS + 1            # pos_encoding rows: noise_steps + 1
TIME_DIM = 256
BOUND = 1e-4
PE = "pos_encoding.pos_encoding"


def _oracle_loss_grad(sd, x, t, cond, noise, scale=None, dtype=torch.float64):
    """float64 autograd through the oracle; with ``scale`` (B, time_dim) the dropout case: pe rows pe[t_b] * scale_b as the
    table, t' = arange(B)."""
    params = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()}
    if scale is not None:
        tb = torch.as_tensor(t).reshape(-1).expand(x.shape[0]) if torch.as_tensor(t).numel() == 1 else torch.as_tensor(t)
        params[PE] = params[PE][tb.long()] * scale.to(dtype)
        t = torch.arange(x.shape[0])
    for k in params:
        if k != PE:
            params[k].requires_grad_(True)
    c = cond.to(dtype).requires_grad_(True)
    fwd = getattr(simple_unet_forward, "__wrapped__", simple_unet_forward)
    with torch.enable_grad():
        eps = fwd(params, x.to(dtype), t, c)
        loss = torch.mean((noise.to(dtype) - eps) ** 2)
        loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in params.items() if k != PE}
    return loss.detach(), eps.detach(), grads, c.grad


def _data(B, H, D, seed, t_mode):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, H, D, generator=g)
    noise = torch.randn(B, 1, H, D, generator=g)
    cond = torch.randn(B, 1, 2, COND_DIM // 2, generator=g)
    t = torch.randint(0, T_ROWS, (1,) if t_mode == "broadcast" else (B,), generator=g)
    return x, t, cond, noise


def _mask(B, seed):
    g = torch.Generator().manual_seed(seed)
    keep = (torch.rand(B, TIME_DIM, generator=g) >= 0.1).float()
    return keep / 0.9                                   # = F.dropout(ones, 0.1, True) for a fixed draw


def _weights(seed):
    return random_state_dict(COND_DIM, seed=seed, model="UNet", noise_steps=NOISE_STEPS)


def _engine(H, D, B, exact, sd):
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    eng = SpdmEngine(H, D, COND_DIM, max_batch=B, model="UNet", num_train_timesteps=T_ROWS, exact_fp32=exact,
                     train_simple=True)
    eng.load_state_dict(sd)
    return eng


def _cls(name):
    if name == "grad_cond":
        return "grad_cond"
    if name.startswith("outc."):
        return "outc"
    if name.endswith(".bias") and "norm." not in name:
        return "bias"
    if "norm." in name:
        return "GroupNorm affine"
    if "cond_emb_layer" in name:
        return "cond_emb_layer"
    if "emb_layer" in name:
        return "emb_layer"
    return "conv weight"


def _check(got, want, what, worst):
    g = got.detach().double().cpu()
    w = want.double()
    den = float(w.norm())
    err = float((g - w).norm())
    if den == 0.0:
        assert err == 0.0, f"{what}: expected exact zeros, |g| = {err:.3e}"
        return
    worst[what] = err / den


def _compare(eng, x, t, cond, noise, ref, scale=None, tag=""):
    loss64, eps64, g64, gc64 = ref
    loss, eps, grads, gcond = eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda(),
                                                time_scale=scale.cuda() if scale is not None else None)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss64)) <= 1e-6 * float(loss64), (float(loss), float(loss64))
    assert float((eps.cpu().double() - eps64).norm()) <= 1e-5 * float(eps64.norm())
    assert set(grads) == set(g64) and PE not in grads
    worst = {}
    for name, want in g64.items():
        _check(grads[name], want, name, worst)
    _check(gcond.reshape(gc64.shape), gc64, "grad_cond", worst)
    per = {}
    for k, v in worst.items():
        per[_cls(k)] = max(per.get(_cls(k), 0.0), v)
    print(f"\nCLASSES {tag}: " + ", ".join(f"{c} {v:.2e}" for c, v in sorted(per.items())))
    bad = {k: v for k, v in worst.items() if not v <= BOUND}
    assert not bad, "||g - g64|| / ||g64|| above %g: %s" % (BOUND, ", ".join(f"{k} {v:.2e}" for k, v in sorted(bad.items())))
    return grads


CASES = [(shape, mode) for shape in ((2, 16, 3), (16, 31, 5), (256, 32, 3), (8, 64, 6)) for mode in ("per_sample", "broadcast")]
_REF = {}


def _reference(case, t_mode):
    if (case, t_mode) not in _REF:
        B, H, D = case
        sd = _weights(11)
        x, t, cond, noise = _data(B, H, D, 5, t_mode)
        _REF[(case, t_mode)] = (sd, x, t, cond, noise, _oracle_loss_grad(sd, x, t, cond, noise))
    return _REF[(case, t_mode)]


@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
@pytest.mark.parametrize("case,t_mode", CASES, ids=[f"B{c[0]}_H{c[1]}_D{c[2]}_{m}" for c, m in CASES])
def test_gradients_match_float64_oracle(case, t_mode, exact):
    B, H, D = case
    sd, x, t, cond, noise, ref = _reference(case, t_mode)
    eng = _engine(H, D, B, exact, sd)
    _compare(eng, x, t, cond, noise, ref, tag=f"{case} {t_mode} {'exact' if exact else 'split'}")
    eng.close()


@pytest.mark.parametrize("case", [(4, 16, 3), (32, 32, 3)], ids=["B4_H16", "B32_H32"])
def test_dropout_time_scale_matches_oracle(case):
    B, H, D = case
    sd = _weights(13)
    x, t, cond, noise = _data(B, H, D, 9, "per_sample")
    scale = _mask(B, 4)
    eng = _engine(H, D, B, False, sd)
    _compare(eng, x, t, cond, noise, _oracle_loss_grad(sd, x, t, cond, noise, scale=scale), scale=scale, tag=f"{case} dropout")
    # the setting is consumed: the next call is the eval-mode network again
    _compare(eng, x, t, cond, noise, _oracle_loss_grad(sd, x, t, cond, noise), tag=f"{case} after dropout")
    eng.close()


def test_edge_data():
    """An all-zero sample, large offsets, and t = 0 and t = T - 1 in one batch."""
    B, H, D = 4, 16, 3
    sd = _weights(17)
    x, _, cond, noise = _data(B, H, D, 6, "per_sample")
    x[0] = 0.0
    noise[0] = 0.0
    cond[0] = 0.0
    x[1] += 30.0
    cond[2] -= 25.0
    t = torch.tensor([0, T_ROWS - 1, 0, T_ROWS - 1])
    eng = _engine(H, D, B, True, sd)
    _compare(eng, x, t, cond, noise, _oracle_loss_grad(sd, x, t, cond, noise), tag="edge")
    eng.close()


def test_deterministic():
    B, H, D = 8, 16, 3
    sd = _weights(2)
    x, t, cond, noise = _data(B, H, D, 1, "per_sample")
    scale = _mask(B, 1).cuda()
    eng = _engine(H, D, B, False, sd)
    for ts in (None, scale):
        a = eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda(), flat=True, time_scale=ts)
        b = eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda(), flat=True, time_scale=ts)
        torch.cuda.synchronize()
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and float(a[0]) == float(b[0])
    eng.close()


def test_batch_gradient_is_mean_of_samples():
    B, H, D = 4, 16, 3
    sd = _weights(6)
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
        if n == PE:
            assert float(gB[off:off + cnt].abs().max()) == 0.0
        elif den > 0:
            assert float((gB[off:off + cnt] - w).norm()) <= BOUND * den, n
    eng.close()


@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact"])
def test_forward_and_sampling_match_plain_simple_handle(exact):
    """Every entry point but spdm_train_loss_grad behaves as on a plain SPDM_FLAG_SIMPLE_UNET handle: bit-identical eps and
    samples."""
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    B, H, D = 8, 32, 3
    sd = _weights(7)
    x, t, cond, _ = _data(B, H, D, 2, "per_sample")
    plain = SpdmEngine(H, D, COND_DIM, max_batch=B, model="UNet", num_train_timesteps=T_ROWS, exact_fp32=exact)
    plain.load_state_dict(sd)
    eng = _engine(H, D, B, exact, sd)
    out = []
    for e in (plain, eng):
        eps = e.unet_forward(x.cuda(), t, cond.cuda()).cpu()
        e.set_builtin_schedule(_lib.SPDM_DDIM, NOISE_STEPS, 10)
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
    TR, TA, TS, SU = _lib.SPDM_FLAG_TRAIN, _lib.SPDM_FLAG_TRAIN_ATTENTION, _lib.SPDM_FLAG_TRAIN_SIMPLE, _lib.SPDM_FLAG_SIMPLE_UNET

    def create(attention, flags):
        cfg = _lib.SpdmConfig(16, 3, COND_DIM, TIME_DIM, attention, 2, 0, T_ROWS, flags)
        h = ctypes.c_void_p()
        rc = lib.spdm_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc == 0:
            lib.spdm_destroy(h)
        return rc

    assert create(0, TR | SU) == -1                           # still refused without the new flag ...
    assert "SPDM_FLAG_TRAIN_SIMPLE" in lib.spdm_last_error().decode()   # ... and the message names it
    assert create(0, TS | SU) == -1                           # the new flag without SPDM_FLAG_TRAIN
    assert create(0, TR | TS) == -1                           # ... without SPDM_FLAG_SIMPLE_UNET
    assert create(1, TR | TS) == -1
    assert create(0, TR | TS | SU | TA) == -1                 # ... with SPDM_FLAG_TRAIN_ATTENTION
    assert create(0, TR | TS | SU) == 0
    with pytest.raises(ValueError):
        SpdmEngine(16, 3, COND_DIM, max_batch=2, attention=False, train_simple=True)
    with pytest.raises(ValueError):
        SpdmEngine(16, 3, COND_DIM, max_batch=2, model="UNet_Film", train_simple=True)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        SpdmEngine(16, 3, COND_DIM, max_batch=2, model="UNet", num_train_timesteps=T_ROWS, train=True)
    sd = _weights(1)
    eng = _engine(16, 3, 2, False, sd)
    x, t, cond, noise = _data(2, 16, 3, 1, "per_sample")
    xs, ns = x.cuda().reshape(2, 16, 3), noise.cuda().reshape(2, 16, 3)
    buf = torch.zeros(eng._blob_floats, device="cuda")
    loss = torch.zeros((), device="cuda")
    tt = t.numpy().astype(np.int32)

    def ptr(z):
        return ctypes.c_void_p(z.data_ptr()) if z is not None else None

    rc = lib.spdm_train_loss_grad(eng._h, 2, ptr(xs), tt.ctypes.data_as(ctypes.c_void_p), 2, None, ptr(ns), ptr(loss), None,
                                  ptr(buf), None, None)
    assert rc == -1 and "d_cond" in lib.spdm_last_error().decode()          # NULL cond
    with pytest.raises(ValueError):                                           # time_scale with the wrong B
        eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda(), time_scale=torch.ones(3, TIME_DIM, device="cuda"))
    scale = torch.ones(1, TIME_DIM, device="cuda")
    assert lib.spdm_train_set_time_scale(eng._h, ptr(scale), 1) == 0
    rc = lib.spdm_train_loss_grad(eng._h, 2, ptr(xs), tt.ctypes.data_as(ctypes.c_void_p), 2, ptr(cond.cuda().reshape(2, -1)),
                                  ptr(ns), ptr(loss), None, ptr(buf), None, None)
    torch.cuda.synchronize()
    assert rc == -1 and "B = 2" in lib.spdm_last_error().decode()
    assert lib.spdm_train_set_time_scale(eng._h, None, 0) == 0                 # NULL clears
    eng.close()
    film = SpdmEngine(16, 3, COND_DIM, max_batch=2, attention=False, num_train_timesteps=NOISE_STEPS, train=True)
    assert lib.spdm_train_set_time_scale(film._h, ptr(scale), 1) == -3         # SPDM_ERR_STATE on a FiLM training handle
    with pytest.raises(ValueError):
        film.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda(), time_scale=scale)
    film.close()


def _facade_batch(B, T, g):
    return {"position": torch.randn(B, T, 2, generator=g), "action": torch.randn(B, T, 3, generator=g),
            "velocity": torch.randn(B, T, 2, generator=g), "image_features": torch.randn(B, T, 4, generator=g)}


def test_training_step_backward_unet_against_oracle():
    """Diffusion_DDPM(model='UNet').training_step(backward=True): loss, grads() over every named parameter and grad_cond
    against float64 oracle autograd, with and without a dropout time_scale; load_state_dict reaches the cached training
    engine."""
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    g = torch.Generator().manual_seed(12)
    obs_h, pred_h, inp_h, B = 3, 13, 3, 4
    kw = dict(noise_steps=50, obs_horizon=obs_h, pred_horizon=pred_h, observation_dim=11, prediction_dim=5, model="UNet",
              inpaint_horizon=inp_h)
    m = Diffusion_DDPM(**kw, weight_seed=3, max_batch=B)
    batch = _facade_batch(B, obs_h + pred_h, g)
    t = torch.tensor([0, 9, 23, 49])
    noise = torch.randn(B, 1, pred_h + inp_h, 5, generator=g)
    obs = {k: v[:, :obs_h].float() for k, v in batch.items()}
    cond = torch.cat([obs["position"], obs["action"], obs["velocity"], obs["image_features"]], -1).unsqueeze(1)
    torch.manual_seed(0)
    mask = F.dropout(torch.ones(B, TIME_DIM, device="cuda"), 0.1, True)
    for ts in (None, mask):
        loss, eps, x_noisy = m.training_step({k: v.clone() for k, v in batch.items()}, t=t, noise=noise, return_parts=True,
                                             backward=True, time_scale=ts)
        assert m._train_engine.train_simple
        assert m._train_engine.num_train_timesteps == m.noise_estimator._sd[PE].shape[0]
        loss64, _, g64, gc64 = _oracle_loss_grad(m.noise_estimator._sd, x_noisy.cpu(), t, cond, noise,
                                                 scale=ts.cpu() if ts is not None else None)
        assert abs(float(loss) - float(loss64)) <= 1e-6 * float(loss64)
        grads = m.noise_estimator.grads()
        assert set(grads) == set(g64) == set(m.noise_estimator._sd) - {PE}
        worst = {}
        for name, want in g64.items():
            _check(grads[name], want, name, worst)
        _check(m.noise_estimator.grad_cond.reshape(gc64.shape), gc64, "grad_cond", worst)
        assert max(worst.values()) <= BOUND, max(worst.items(), key=lambda kv: kv[1])
    sd2 = {k: (v * 0.5 if k != PE else v) for k, v in m.noise_estimator._sd.items()}
    m.noise_estimator.load_state_dict(sd2)
    loss2, eps2, _ = m.training_step({k: v.clone() for k, v in batch.items()}, t=t, noise=noise, return_parts=True,
                                     backward=True)
    want2 = simple_unet_forward(sd2, x_noisy.cpu(), t, cond)
    assert float((eps2.cpu() - want2).abs().max()) <= 1e-4
    assert abs(float(loss2) - float(torch.mean((noise - want2) ** 2))) <= 1e-5
    with pytest.raises(ValueError):
        m.training_step(batch, t=t, noise=noise, time_scale=mask)                      # forward only
    with pytest.raises(ValueError):
        Diffusion_DDPM(**dict(kw, model="UNet_FilmnoAttention")).training_step(batch, t=t, noise=noise, backward=True,
                                                                                 time_scale=mask)
    with pytest.raises(NotImplementedError, match="train_attention"):
        Diffusion_DDPM(**dict(kw, model="UNet_Film")).training_step(batch, t=t, noise=noise, backward=True)


def test_short_adam_run_tracks_fp32_oracle():
    """20 torch-Adam steps (lr 1e-3, fixed data) on the HIP gradients and on fp32 oracle autograd from the same start."""
    B, H, D = 8, 16, 3
    sd0 = _weights(8)
    x, t, cond, noise = _data(B, H, D, 4, "per_sample")
    names = [n for n in sd0 if n != PE]
    shapes = [np.asarray(sd0[n]).shape for n in names]
    flat0 = torch.cat([torch.as_tensor(np.asarray(sd0[n])).reshape(-1) for n in names])

    def unflat(v):
        out, off = {PE: sd0[PE]}, 0
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
        loss, _, g, _ = eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda())
        p_hip.grad = torch.cat([g[n].reshape(-1) for n in names])
        opt_hip.step()
        lr, _, gr, _ = _oracle_loss_grad(unflat(p_ref.detach()), x, t, cond, noise, dtype=torch.float32)
        p_ref.grad = torch.cat([gr[n].reshape(-1) for n in names])
        opt_ref.step()
        lh, lr_ = float(loss), float(lr)
        assert abs(lh - lr_) <= 1e-3 * lr_, (step, lh, lr_)
        losses.append(lh)
    assert losses[-1] < losses[0]
    eng.close()
