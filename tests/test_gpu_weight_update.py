"""In-place weight update (spdm_update_weights / SpdmEngine.update_weights): a handle loaded with sd0 and
updated to sd1 holds, bit for bit, what a fresh handle loaded with sd1 holds -- every device weight copy at once
(spdm_debug_weight_digest) and the outputs of every route; range changes are refused and fall back to a rebuild; the facade's
optimiser step (configure_optimizers + optimizer_step) equals the same clip + Adam loop over the rebuild path."""
import ctypes

import numpy as np
import pytest
import torch

from state_policy_diffusionmodel_amd import _lib
from state_policy_diffusionmodel_amd.engine import SpdmEngine
from state_policy_diffusionmodel_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

H, D, COND, T_SIMPLE = 32, 3, 60, 1000
KINDS = {
    "attn_split": dict(attention=True),
    "attn_exact": dict(attention=True, exact_fp32=True),
    "noattn": dict(attention=False),
    "simple_split": dict(model="UNet"),
    "simple_exact": dict(model="UNet", exact_fp32=True),
    "train_noattn": dict(attention=False, train=True),
    "train_attn": dict(attention=True, train_attention=True),
    "train_simple": dict(model="UNet", train_simple=True),
}


def _sd(kind, seed):
    kw = KINDS[kind]
    if kw.get("model") == "UNet":
        return random_state_dict(COND, seed=seed, model="UNet", noise_steps=T_SIMPLE)
    return random_state_dict(COND, seed=seed, attention=kw["attention"])


def _engine(kind, sd, max_batch=4, **extra):
    kw = dict(KINDS[kind])
    kw.update(extra)
    if kw.get("model") == "UNet":
        kw["num_train_timesteps"] = T_SIMPLE + 1
    eng = SpdmEngine(H, D, COND, max_batch=max_batch, **kw)
    eng.load_state_dict(sd)
    return eng


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, H, D, generator=g).cuda()
    cond = torch.randn(B, 1, COND, generator=g).cuda()
    noise = torch.randn(B, 1, H, D, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g)
    return x, cond, noise, t


def _raw_update(eng, flat, n=None):
    return eng.lib.spdm_update_weights(eng._h, ctypes.c_void_p(flat.data_ptr()), flat.numel() if n is None else n,
                                       eng._stream())


def _assert_same_forward(a, b, B, seed):
    x, cond, _, t = _inputs(B, seed)
    torch.cuda.synchronize()
    for tt in (t, t[:1]):                       # per-sample and broadcast t
        ea, eb = a.unet_forward(x, tt, cond), b.unet_forward(x, tt, cond)
        assert torch.equal(ea, eb)


@pytest.mark.parametrize("kind", list(KINDS))
def test_update_equals_fresh_load(kind):
    sd0, sd1 = _sd(kind, 0), _sd(kind, 1)
    a = _engine(kind, sd0)
    d0 = a.weight_digest()
    ptr, nbytes = a._h.value, a.device_bytes
    a.update_weights(a.pack_weights(sd1))
    b = _engine(kind, sd1)
    assert a.weight_digest() == b.weight_digest() != d0
    assert a._h.value == ptr and a.device_bytes == nbytes and a.weight_rebuilds == 0
    if a.train:
        x, cond, noise, t = _inputs(4, 3)
        ts = (torch.nn.functional.dropout(torch.ones(4, 256, device="cuda"), 0.1, True) if kind == "train_simple" else None)
        ra = a.loss_and_grad(x, t, cond, noise, flat=True, time_scale=ts)
        rb = b.loss_and_grad(x, t, cond, noise, flat=True, time_scale=ts)
        for u, v in zip(ra, rb):
            assert torch.equal(u, v)
    else:
        _assert_same_forward(a, b, 1, 4)
    a.close()
    b.close()


@pytest.mark.parametrize("kind", ["attn_split", "noattn", "simple_split"])
def test_update_equals_fresh_load_large_batch(kind):
    """B = 1024 takes the wide / reg64 / sa_tail / sa_head routes; their weight copies must be the fresh ones too."""
    sd0, sd1 = _sd(kind, 0), _sd(kind, 5)
    a = _engine(kind, sd0, max_batch=1024)
    a.update_weights(a.pack_weights(sd1))
    b = _engine(kind, sd1, max_batch=1024)
    assert a.weight_digest() == b.weight_digest()
    _assert_same_forward(a, b, 1024, 6)
    _assert_same_forward(a, b, 1, 7)
    a.close()
    b.close()


def test_sampling_graph_captured_before_update():
    """A DDPM loop whose step graph was captured before the update (the graph bakes outc's bias in) equals a fresh handle's."""
    sd0, sd1 = _sd("attn_split", 0), _sd("attn_split", 1)
    sd1["outc.bias"] = sd0["outc.bias"] + np.float32(0.25)
    a = _engine("attn_split", sd0)
    b = _engine("attn_split", sd1)
    for e in (a, b):
        e.set_builtin_schedule(_lib.SPDM_DDPM, 1000, 12)
    x, cond, _, _ = _inputs(2, 8)
    a.sample(cond, x, seed=3)
    assert a.graph_captures == 1
    a.update_weights(a.pack_weights(sd1))
    assert torch.equal(a.sample(cond, x, seed=3), b.sample(cond, x, seed=3))
    assert a.graph_captures == 2
    # the same bias again: the graph is kept
    a.update_weights(a.pack_weights(sd1))
    assert torch.equal(a.sample(cond, x, seed=3), b.sample(cond, x, seed=3))
    assert a.graph_captures == 2
    a.close()
    b.close()


def _edge(sd, names):
    """zeros, subnormals, +-510.99 and fp16 rounding ties of 128 w (in hi and in the subnormal fp16 range)"""
    vals = np.array([0.0, -0.0, 1e-40, -3e-39, 510.99, -510.99, (1 + 2.0 ** -11) / 128, -(1 + 3 * 2.0 ** -11) / 128,
                     1.5 * 2.0 ** -24 / 128, 2.5 * 2.0 ** -24 / 128, 2.0 ** -30, 1e-45], dtype=np.float32)
    sd = dict(sd)
    for n in names:
        w = sd[n].copy().reshape(-1)
        w[:vals.size] = vals
        w[-vals.size:] = -vals[::-1]
        sd[n] = w.reshape(sd[n].shape)
    return sd


@pytest.mark.parametrize("kind", ["attn_split", "simple_split"])
def test_edge_values(kind):
    sd0 = _sd(kind, 0)
    if kind == "attn_split":
        names = ["down1.doubleConv1.first.weight", "down3.doubleConv2.second.weight", "sa5.attention.in_proj_weight",
                 "sa1.attention.out_proj.weight", "up1.cond_encoder.2.weight", "up2.emb_layer.1.weight", "inc.first.weight"]
    else:
        names = ["down1.doubleConv1.first.weight", "up1.doubleConv1.first.weight", "down2.cond_emb_layer.1.weight",
                 "up3.emb_layer.1.weight", "input_conv.first.weight"]
    sd1 = _edge(_sd(kind, 1), names)
    a = _engine(kind, sd0)
    a.update_weights(a.pack_weights(sd1))
    b = _engine(kind, sd1)
    assert a.demoted_tensors == b.demoted_tensors == 0
    assert a.weight_digest() == b.weight_digest()
    _assert_same_forward(a, b, 2, 9)
    a.close()
    b.close()


@pytest.mark.parametrize("name,value", [("down2.doubleConv1.second.weight", 600.0),
                                        ("sa5.attention.in_proj_weight", -512.0),
                                        ("up1.doubleConv2.first.weight", float("nan"))])
def test_range_change_is_refused_then_rebuilt(name, value):
    sd1 = _sd("attn_split", 1)
    a = _engine("attn_split", sd1)
    d1 = a.weight_digest()
    x, cond, _, t = _inputs(2, 10)
    e1 = a.unet_forward(x, t, cond)
    sd2 = dict(sd1)
    w = sd2[name].copy()
    w.reshape(-1)[7] = value
    sd2[name] = w
    flat2 = a.pack_weights(sd2)
    assert _raw_update(a, flat2) == -3
    assert name.encode() in a.lib.spdm_last_error()
    assert a.weight_digest() == d1 and a.demoted_tensors == 0
    assert torch.equal(a.unet_forward(x, t, cond), e1)
    a.update_weights(flat2)                           # falls back to a rebuild
    assert a.weight_rebuilds == 1 and a.demoted_tensors == 1
    b = _engine("attn_split", sd2)
    assert a.weight_digest() == b.weight_digest()
    if value == value:                                # (a NaN weight gives NaN outputs on both)
        _assert_same_forward(a, b, 2, 11)
    # ... and back into the range: refused the same way
    assert _raw_update(a, a.pack_weights(sd1)) == -3
    a.close()
    b.close()


def test_refusals_and_session():
    sd0, sd1 = _sd("noattn", 0), _sd("noattn", 1)
    raw = SpdmEngine(H, D, COND, max_batch=2, attention=False)
    flat = torch.zeros(16, device="cuda")
    assert _raw_update(raw, flat) == -3                # before load
    raw.close()
    a = _engine("noattn", sd0)
    flat1 = a.pack_weights(sd1)
    assert _raw_update(a, flat1, flat1.numel() - 1) == -1
    assert a.lib.spdm_update_weights(a._h, None, flat1.numel(), a._stream()) == -1
    with pytest.raises(ValueError):
        a.pack_weights({k: v for k, v in list(sd1.items())[1:]})
    a.set_builtin_schedule(_lib.SPDM_DDPM, 1000, 5)
    x, cond, _, _ = _inputs(2, 12)
    a.sample_begin(cond, x)
    ptr, nbytes = a._h.value, a.device_bytes
    assert _raw_update(a, flat1) == 0
    assert a.lib.spdm_sample_run(a._h, 0, 5, a._stream()) == -3
    assert a._h.value == ptr and a.device_bytes == nbytes
    b = _engine("noattn", sd1)
    b.set_builtin_schedule(_lib.SPDM_DDPM, 1000, 5)
    assert torch.equal(a.sample(cond, x, seed=1), b.sample(cond, x, seed=1))
    a.close()
    b.close()


def _facade_batch(B, T, g):
    return {"position": torch.randn(B, T, 2, generator=g), "action": torch.randn(B, T, 3, generator=g),
            "velocity": torch.randn(B, T, 2, generator=g), "image_features": torch.randn(B, T, 4, generator=g)}


@pytest.mark.parametrize("model", ["UNet_FilmnoAttention", "UNet_Film", "UNet"])
def test_training_loop_matches_rebuild_path(model):
    """20 steps of configure_optimizers + training_step(backward=True) + optimizer_step(opt, 0.5) equal, bit for bit, the
    same clip + Adam whose weights reach the training engine through SpdmEngine.refresh_weights."""
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    obs_h, pred_h, inp_h, B, steps = 3, 13, 3, 4, 20
    kw = dict(noise_steps=50, obs_horizon=obs_h, pred_horizon=pred_h, observation_dim=11, prediction_dim=5, model=model,
              inpaint_horizon=inp_h, weight_seed=3, max_batch=B, learning_rate=1e-3, train_attention=model == "UNet_Film")
    g = torch.Generator().manual_seed(21)
    data = []
    for _ in range(steps):
        batch = _facade_batch(B, obs_h + pred_h, g)
        t = torch.randint(0, 50, (B,), generator=g)
        noise = torch.randn(B, 1, pred_h + inp_h, 5, generator=g)
        scale = (torch.rand(B, 256, generator=g) >= 0.1).float() / 0.9 if model == "UNet" else None
        data.append((batch, t, noise, scale))

    def step_args(i):
        batch, t, noise, scale = data[i]
        return dict(batch={k: v.clone() for k, v in batch.items()}, t=t, noise=noise, backward=True,
                    time_scale=scale.cuda() if scale is not None else None)

    # the facade: in-place updates
    m = Diffusion_DDPM(**kw)
    x0, cond = torch.randn(B, 1, pred_h + inp_h, 5, generator=g), torch.randn(B, 1, obs_h, 11, generator=g)
    m.noise_estimator(x0.cuda(), torch.tensor([7]), cond.cuda())         # a cached sampling engine receives the updates too
    opt = m.configure_optimizers()["optimizer"]
    losses = []
    for i in range(steps):
        losses.append(m.training_step(**step_args(i)).clone())
        m.optimizer_step(opt, 0.5)
    p = m.noise_estimator.flat_parameter()
    assert m._train_engine.weight_rebuilds == 0

    # the rebuild path: the same clip + Adam over a flat parameter of our own
    r = Diffusion_DDPM(**kw)
    eng = r._train_engine_for(B, pred_h + inp_h, 5)
    q = torch.nn.Parameter(eng.pack_weights(r.noise_estimator._sd))
    opt2 = torch.optim.Adam([q], lr=1e-3)
    for i in range(steps):
        loss = r.training_step(**step_args(i))
        assert torch.equal(loss, losses[i]), i
        grad = torch.zeros_like(q)
        for name, off, shape in eng._index:
            gr = r.noise_estimator.grads().get(name)
            if gr is not None:
                grad[off:off + gr.numel()] = gr.reshape(-1)
        q.grad = grad
        torch.nn.utils.clip_grad_norm_([q], 0.5)
        opt2.step()
        eng.refresh_weights(eng.unpack_weights(q.detach()))
    assert torch.equal(p.detach(), q.detach())

    # the sampling engine took every update: its eps equals a fresh engine's on state_dict()
    sd = m.noise_estimator.state_dict()
    fresh = SpdmEngine(pred_h + inp_h, 5, m.cond_dim, max_batch=B, attention=m.attention,
                       num_train_timesteps=m._engine.num_train_timesteps, model="UNet" if m.simple else None)
    fresh.load_state_dict(sd)
    tt = torch.tensor([7])
    assert torch.equal(m.noise_estimator(x0.cuda(), tt, cond.cuda()), fresh.unet_forward(x0.cuda(), tt, cond.cuda()))
    assert m._engine.weight_digest() == fresh.weight_digest()
    fresh.close()
