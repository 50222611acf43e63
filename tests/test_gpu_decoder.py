"""The autoencoder's decoder and its reconstruction training on the HIP path (spdm_decoder_*, autoencoder.Decoder and the
``autoencoder`` facade) against float64 autograd through tests/autoencoder_ref.py.

Bounds are the project's: TOL 1e-4 absolute on values, BOUND 1e-4 on ||g - g64||_2 / ||g64||_2 per tensor, 1e-6 relative
on the loss; the short Adam run's loss within 1e-3 relative per step of the same loop in torch-CPU fp32
(tests/test_gpu_encoder_joint.py's bound).  Latents are 0.3 N(0,1) with one row of zeros, targets and frames U[0,1) with
a zero corner patch and a last row of ones.  The float64 reference picks its own ReLU masks.  On the n = 130 decoder case
one a1 unit's fp32 pre-activation is -7.5e-9 where float64 gives +2.2e-8; with the fp32 forward's masks that moved 0.weight /
0.bias / 2.weight / grad_latent by 3.8e-4 / 2.7e-4 / 2.3e-4 / 3.6e-4 (torch-CPU fp32 autograd misses float64 by the same
figures), so train_loss settles the saved maps' signs in float64 (decoder_kinks_kernel).

Measured (MI355X), worst ratio per tensor.  Decoder alone over n = 1, 6, 40, 130: 0.weight 2.5e-7, 0.bias 2.0e-7,
2.weight 3.1e-7, 2.bias 9.9e-8, 4.weight 2.3e-7, 4.bias 1.7e-7, 6.weight 6.4e-8, 6.bias 9.5e-8, grad_latent 1.7e-6, loss
4.1e-8; forward 6.4e-8 absolute against float64, 6.0e-8 against fp32 CPU at n = 2100.  Through the facade: encoder tensors
<= 4.0e-6, decoder tensors <= 1.1e-6, loss <= 2.1e-8.  n = 2100 against its 128-frame pieces: tensors <= 4.2e-7,
grad_latent 2.4e-6, loss 2.3e-8.  After update_weights <= 2.8e-7 (grad_latent 1.8e-6).  Adam run: 0, 0, 8.8e-8, 8.8e-8, 0
relative over its five steps.

The (flavour, n) cases run the same two gradient tests on trained-scale data (autoencoder_ref.TRAINED_CASES):
layer 6 scaled by 40 / 120 so that the sigmoid saturates, the encoder's convolutions by 3 with dead channels, 8-bit frames with a
black band on the padded border and flat patches.  Measured: decoder tensors <= 7.8e-7, grad_latent 1.9e-6, loss 4.5e-8;
through the facade all 16 tensors <= 1.3e-6, loss 4.6e-8.
"""
import ctypes
import functools

import pytest
import torch

from autoencoder_ref import (DEC_KEYS, TRAINED_CASES, autoencoder_grads, case_id, decoder_forward_any, decoder_grads, latents,
                             make_decoder_state_dict, trained_decoder_state_dict, trained_encoder_state_dict, trained_frames)
from encoder_train_ref import KEYS as ENC_KEYS
from encoder_train_ref import encoder_forward_any, images
from oracle.encoder_ref import make_encoder_state_dict

pytestmark = pytest.mark.gpu

BOUND = 1e-4
TOL = 1e-4
LOSS_REL = 1e-6
DEC_SEED, ENC_SEED = 6, 5


def _decoder(seed=DEC_SEED):
    from state_policy_diffusionmodel_amd.autoencoder import Decoder
    sd = make_decoder_state_dict(seed)
    return sd, Decoder(sd)


def _checkpoint(enc_sd, dec_sd):
    sd = {"encoder." + k: v for k, v in enc_sd.items()}
    sd.update({"decoder." + k: v for k, v in dec_sd.items()})
    return sd


def _dec_sd(case):
    """torch's default initialisation for a frame count; layer 6 scaled by 40 / 120 for a (flavour, n) pair of TRAINED_CASES"""
    return make_decoder_state_dict(DEC_SEED) if isinstance(case, int) else trained_decoder_state_dict(DEC_SEED, int(case[0][7:]))


@functools.lru_cache(maxsize=None)
def _inputs(case):
    if isinstance(case, int):
        return latents(case, 10 + case), images(case, 200 + case)
    return latents(case[1], 10 + case[1]), trained_frames(case[1], 200 + case[1])


@functools.lru_cache(maxsize=None)
def _ref64(case):
    """float64 reconstruction, loss, gradients and grad_latent of the decoder on _inputs(case): computed once, read only."""
    z, tgt = _inputs(case)
    sd = _dec_sd(case)
    recon = decoder_forward_any({k: v.double() for k, v in sd.items()}, z.double())
    loss, grads, gl = decoder_grads(sd, z, tgt)
    return recon, loss, grads, gl


def _ratios(got, want, keys, prefix=""):
    out = {}
    for k in keys:
        g, w = got[k].detach().double().cpu(), want[k].double().cpu()
        assert g.shape == w.shape, k
        if float(w.norm()) == 0.0:             # (n = 1: the one latent row is the zero row, so 0.weight's gradient is exactly zero)
            assert float(g.abs().max()) == 0.0, k
            out[prefix + k] = 0.0
        else:
            out[prefix + k] = float((g - w).norm() / w.norm())
    return out


def _assert_within(tag, worst):
    print(f"\nDECODER GRAD {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= BOUND}
    assert not bad, "||g - ref|| / ||ref|| above %g: %s" % (BOUND, ", ".join(f"{k} {v:.2e}" for k, v in sorted(bad.items())))


@pytest.mark.parametrize("n", [1, 7, 130])
def test_forward_matches_float64(n):
    """n = 7: a partial 128-row tile at every layer; n = 130: the Linear's rows cross a tile."""
    sd, dec = _decoder()
    try:
        z = latents(n, 10 + n)
        want = decoder_forward_any({k: v.double() for k, v in sd.items()}, z.double())
        got = dec(z.cuda())
        assert got.shape == (n, 3, 96, 96)
        err = float((got.cpu().double() - want).abs().max())
        print(f"\nDECODER FORWARD n={n}: max abs {err:.2e}")
        assert err <= TOL
    finally:
        dec.close()


def test_forward_across_the_chunk_matches_fp32_cpu():
    """n = 2100 crosses the 2048-frame chunk."""
    sd, dec = _decoder()
    try:
        z = latents(2100, 3)
        with torch.no_grad():
            want = decoder_forward_any(sd, z)
        err = float((dec(z.cuda()).cpu() - want).abs().max())
        print(f"\nDECODER FORWARD n=2100 vs fp32 CPU: max abs {err:.2e}")
        assert err <= TOL
    finally:
        dec.close()


@pytest.mark.parametrize("n", [1, 7, 2100])
def test_train_loss_recon_equals_forward_bit_for_bit(n):
    sd, dec = _decoder()
    try:
        z, tgt = latents(n, n).cuda(), images(n, n).cuda()
        dec.train_loss(z, tgt)
        assert torch.equal(dec.recon, dec(z))
    finally:
        dec.close()


@pytest.mark.parametrize("n", [1, 6, 40, 130, *TRAINED_CASES], ids=case_id)
def test_decoder_gradients_match_float64_autograd(n):
    """The (flavour, n) cases: layer 6 scaled by 40 / 120 (a saturated sigmoid) against 8-bit frames with flat patches."""
    from state_policy_diffusionmodel_amd.autoencoder import Decoder
    dec = Decoder(_dec_sd(n))
    try:
        z, tgt = _inputs(n)
        recon64, loss64, g64, gl64 = _ref64(n)
        loss = dec.train_loss(z.cuda(), tgt.cuda())
        assert float((dec.recon.cpu().double() - recon64).abs().max()) <= TOL
        rel = abs(float(loss.double()) - loss64) / loss64
        flat, gl = dec.backward()
        torch.cuda.synchronize()
        grads = dec.grads()
        assert set(grads) == set(DEC_KEYS)
        lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
        assert all(lo <= grads[k].data_ptr() < hi for k in DEC_KEYS)              # views of the flat gradient
        assert int(sum(v.numel() for v in grads.values())) == flat.numel()
        worst = _ratios(grads, g64, DEC_KEYS)
        worst.update(_ratios({"grad_latent": gl}, {"grad_latent": gl64}, ["grad_latent"]))
        print(f"\nDECODER LOSS n={case_id(n)}: rel {rel:.2e}")
        _assert_within(f"n={case_id(n)}", worst)
        assert rel <= LOSS_REL
    finally:
        dec.close()


@pytest.mark.parametrize("n", [1, 6, 40, 130, *TRAINED_CASES], ids=case_id)
def test_autoencoder_step_matches_float64_autograd(n):
    """The whole reconstruction step through the facade: all 16 tensors.  The (flavour, n) cases: encoder convolutions scaled by
    3 with dead channels, layer 6 scaled by 40 / 120, 8-bit frames with a black band on the border and flat patches."""
    from state_policy_diffusionmodel_amd.autoencoder import autoencoder
    enc_sd, dec_sd = make_encoder_state_dict(ENC_SEED), _dec_sd(n)
    tag = case_id(n)
    if not isinstance(n, int):
        enc_sd, n = trained_encoder_state_dict(enc_sd), n[1]
    ae = autoencoder(state_dict=_checkpoint(enc_sd, dec_sd))
    try:
        x = images(n, 100 + n) if tag == str(n) else trained_frames(n, 100 + n)
        loss64, e64, d64 = autoencoder_grads(enc_sd, dec_sd, x)
        loss = ae.training_step(x.cuda(), backward=True)
        torch.cuda.synchronize()
        rel = abs(float(loss.double()) - loss64) / loss64
        eg, dg = ae.encoder.grads(), ae.decoder.grads()
        assert set(eg) == set(ENC_KEYS) and set(dg) == set(DEC_KEYS)
        for handle, grads in ((ae.encoder, eg), (ae.decoder, dg)):
            flat = handle.flat_parameter().grad
            assert flat is not None
            lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
            assert all(lo <= g.data_ptr() < hi for g in grads.values())           # views of the flat gradients
        worst = _ratios(eg, e64, ENC_KEYS, "enc/")
        worst.update(_ratios(dg, d64, DEC_KEYS, "dec/"))
        print(f"\nAUTOENCODER LOSS n={tag}: rel {rel:.2e}")
        _assert_within(f"autoencoder n={tag}", worst)
        assert rel <= LOSS_REL
        # validation_step / forward: the same loss without a backward pass, reconstructions in [0, 1]
        assert abs(float(ae.validation_step(x.cuda())) - float(loss)) <= LOSS_REL * float(loss)
        recon = ae(x.cuda())
        with torch.no_grad():
            want = decoder_forward_any(dec_sd, encoder_forward_any(enc_sd, x))
        assert float((recon.cpu() - want).abs().max()) <= TOL
    finally:
        ae.close()


def test_large_n_equals_the_weighted_sum_of_small_runs():
    """n = 2100 (two chunks, the second accumulated onto the first) against sum_p (n_p / n) x this decoder's own gradient
    on 128-frame piece p, which the small-n cases above tie to float64.  The forward is per-frame deterministic, so the
    ReLU masks are the same on both sides; the two differ in fp32 summation order only."""
    sd, dec = _decoder()
    try:
        n = 2100
        z, tgt = latents(n, 4).cuda(), images(n, 5).cuda()
        loss = float(dec.train_loss(z, tgt))
        _, gl = dec.backward()
        full = {k: v.double().clone() for k, v in dec.grads().items()}
        full["grad_latent"] = gl.double().clone()
        acc = {k: torch.zeros_like(v) for k, v in full.items()}
        lsum = 0.0
        for i in range(0, n, 128):
            zi, ti = z[i:i + 128].contiguous(), tgt[i:i + 128].contiguous()
            w = zi.shape[0] / n
            lsum += w * float(dec.train_loss(zi, ti))
            _, gli = dec.backward()
            for k, v in dec.grads().items():
                acc[k] += w * v.double()
            acc["grad_latent"][i:i + 128] = w * gli.double()
        print(f"\nDECODER LOSS n=2100 vs pieces: rel {abs(loss - lsum) / lsum:.2e}")
        _assert_within("n=2100 vs pieces", _ratios(full, acc, list(full)))
        assert abs(loss - lsum) <= LOSS_REL * lsum
    finally:
        dec.close()


def test_determinism_and_call_order():
    from state_policy_diffusionmodel_amd import _lib
    sd, dec = _decoder()
    try:
        n = 40
        z, tgt = latents(n, 1).cuda(), images(n, 2).cuda()
        with pytest.raises(RuntimeError, match=r"\(-3\)"):                 # SPDM_ERR_STATE: no train_loss yet
            dec.backward()
        la = dec.train_loss(z, tgt).clone()
        a, gla = (t.clone() for t in dec.backward())
        with pytest.raises(RuntimeError, match=r"\(-3\)"):                 # one backward per train_loss
            dec.backward()
        lb = dec.train_loss(z, tgt).clone()
        b, glb = dec.backward()
        assert torch.equal(la, lb) and torch.equal(a, b) and torch.equal(gla, glb)

        def raw_backward(count):
            return dec.lib.spdm_decoder_backward(dec._h, count, ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(tgt.data_ptr()),
                                                 ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(gla.data_ptr()), None)
        dec.train_loss(z, tgt)
        dec.update_weights(dec.flat_parameter().detach())
        assert raw_backward(n) == _lib.SPDM_ERR_STATE                      # an update in between invalidates the maps
        dec.train_loss(z, tgt)
        assert raw_backward(n - 1) == _lib.SPDM_ERR_STATE                  # another n
        assert raw_backward(n) == 0                                        # ... which left the pending pass alone
    finally:
        dec.close()


def test_invalid_arguments():
    from state_policy_diffusionmodel_amd import _lib
    from state_policy_diffusionmodel_amd.weights import pack_state_dict
    sd, dec = _decoder()
    try:
        lib = dec.lib
        blob = dec.flat_parameter().detach()
        assert lib.spdm_decoder_update_weights(dec._h, ctypes.c_void_p(blob.data_ptr()), blob.numel() - 1, None) == _lib.SPDM_ERR_INVALID
        z, out = latents(2, 1).cuda(), torch.empty(2, 3, 96, 96, device="cuda")
        assert lib.spdm_decoder_forward(dec._h, 0, ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(out.data_ptr()), None) == _lib.SPDM_ERR_INVALID
        assert lib.spdm_decoder_forward(dec._h, 2, None, ctypes.c_void_p(out.data_ptr()), None) == _lib.SPDM_ERR_INVALID
        assert lib.spdm_decoder_train_loss(dec._h, 2, ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(out.data_ptr()), None, None, None) == _lib.SPDM_ERR_INVALID

        def create(bad_sd):
            b, idx = pack_state_dict(bad_sd)
            h = ctypes.c_void_p()
            rc = lib.spdm_decoder_create(0, b.ctypes.data_as(ctypes.c_void_p), b.size, idx, len(idx), ctypes.byref(h))
            assert not h.value
            return rc
        renamed = {("7.bias" if k == "6.bias" else k): v for k, v in sd.items()}
        assert create(renamed) == _lib.SPDM_ERR_INVALID                    # a wrong name
        reshaped = dict(sd, **{"2.weight": sd["2.weight"].permute(1, 0, 2, 3).contiguous()})
        assert create(reshaped) == _lib.SPDM_ERR_INVALID                   # (32, 64, 2, 2): Conv2d's layout, not ConvTranspose2d's
    finally:
        dec.close()


def test_update_weights_equals_a_fresh_handle():
    from state_policy_diffusionmodel_amd.autoencoder import Decoder
    from state_policy_diffusionmodel_amd.weights import pack_state_dict
    sd, dec = _decoder(DEC_SEED)
    new = make_decoder_state_dict(DEC_SEED + 1)
    fresh = Decoder(new)
    try:
        n = 7
        z, tgt = latents(n, 4).cuda(), images(n, 4).cuda()
        dec.train_loss(z, tgt)                                             # a training handle: the gradient's weight copy follows too
        dec.backward()
        blob, _ = pack_state_dict({k: new[k] for k in DEC_KEYS})
        dec.update_weights(torch.from_numpy(blob).cuda())
        assert torch.equal(dec(z), fresh(z))
        assert all(torch.equal(dec.state_dict()[k], new[k]) for k in DEC_KEYS)
        loss64, g64, gl64 = decoder_grads(new, z.cpu(), tgt.cpu())
        loss = dec.train_loss(z, tgt)
        _, gl = dec.backward()
        worst = _ratios(dec.grads(), g64, DEC_KEYS)
        worst.update(_ratios({"grad_latent": gl}, {"grad_latent": gl64}, ["grad_latent"]))
        _assert_within("after update", worst)
        assert abs(float(loss) - loss64) <= LOSS_REL * loss64
    finally:
        dec.close()
        fresh.close()


def test_adam_run_tracks_fp32_autograd_and_the_checkpoint_feeds_the_diffusion_model():
    from state_policy_diffusionmodel_amd.autoencoder import autoencoder
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    enc_sd, dec_sd = make_encoder_state_dict(3), make_decoder_state_dict(4)
    ae = autoencoder(learning_rate=1e-3, state_dict=_checkpoint(enc_sd, dec_sd))
    try:
        n = 16
        x = images(n, 77)
        cfg = ae.configure_optimizers()
        opt = cfg["optimizer"]
        assert cfg["lr_scheduler"]["monitor"] == "val_loss"
        assert [p is q for p, q in zip(opt.param_groups[0]["params"], (ae.encoder.flat_parameter(), ae.decoder.flat_parameter()))] == [True, True]
        # the same loop in torch-CPU fp32: one Adam over both halves, global-norm clip 0.5
        ref_e = {k: enc_sd[k].clone().requires_grad_(True) for k in ENC_KEYS}
        ref_d = {k: dec_sd[k].clone().requires_grad_(True) for k in DEC_KEYS}
        ref_params = list(ref_e.values()) + list(ref_d.values())
        ref_opt = torch.optim.Adam(ref_params, lr=1e-3)
        losses = []
        xg = x.cuda()
        for step in range(5):
            loss = float(ae.training_step(xg, step, backward=True))
            ae.optimizer_step(opt, gradient_clip_val=0.5)
            ref_opt.zero_grad()
            with torch.enable_grad():
                lr = torch.mean((decoder_forward_any(ref_d, encoder_forward_any(ref_e, x)) - x) ** 2)
                lr.backward()
            torch.nn.utils.clip_grad_norm_(ref_params, 0.5)
            ref_opt.step()
            lr = float(lr.detach())
            print(f"\nAUTOENCODER ADAM step {step}: hip {loss:.7f} ref {lr:.7f} rel {abs(loss - lr) / lr:.2e}")
            assert abs(loss - lr) <= 1e-3 * lr, (step, loss, lr)
            losses.append(loss)
        assert losses[-1] < losses[0]
        sd = ae.state_dict()
        assert set(sd) == {p + h + k for p in ("model.", "") for h, keys in (("encoder.", ENC_KEYS), ("decoder.", DEC_KEYS)) for k in keys}
        assert all(not torch.equal(sd["encoder." + k], enc_sd[k]) for k in ENC_KEYS)
        assert all(not torch.equal(sd["decoder." + k], dec_sd[k]) for k in DEC_KEYS)
        # the trained checkpoint, unchanged, as the diffusion model's frozen encoder
        obs_h, pred_h, B = 2, 14, 2
        m = Diffusion_DDPM(noise_steps=50, obs_horizon=obs_h, pred_horizon=pred_h, observation_dim=135, prediction_dim=3,
                           model="UNet_FilmnoAttention", inpaint_horizon=2, max_batch=B, weight_seed=2,
                           vision_encoder_state_dict=sd)
        g = torch.Generator().manual_seed(9)
        T = obs_h + pred_h
        batch = {"position": torch.randn(B, T, 2, generator=g), "action": torch.randn(B, T, 1, generator=g),
                 "velocity": torch.randn(B, T, 4, generator=g), "image": torch.rand(B, T, 3, 96, 96, generator=g)}
        got = m.prepare_obs_cond_vectors(m.prepare_observation_batch(batch))
        want = ae.encoder(batch["image"][:, :obs_h].flatten(end_dim=1).cuda()).reshape(B, obs_h, 128)
        assert torch.equal(got.reshape(B, obs_h, -1)[..., -128:], want)
        # a round trip through a checkpoint file
        import os
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "autoencoder.ckpt")
            torch.save({"state_dict": sd}, path)
            again = autoencoder.load_from_checkpoint(path)
            try:
                assert torch.equal(again(xg), ae(xg))
            finally:
                again.close()
    finally:
        ae.close()


def test_default_initialisation_has_torch_bounds():
    from state_policy_diffusionmodel_amd.autoencoder import autoencoder
    torch.manual_seed(0)
    ae = autoencoder()
    try:
        sd = ae.state_dict()
        for key, fan_in in (("encoder.0", 12), ("encoder.7", 9216), ("decoder.0", 128), ("decoder.2", 128), ("decoder.4", 64), ("decoder.6", 12)):
            b = 1.0 / fan_in ** 0.5
            assert float(sd[key + ".weight"].abs().max()) <= b and float(sd[key + ".bias"].abs().max()) <= b
            assert float(sd[key + ".weight"].abs().max()) > 0.5 * b
        assert torch.isfinite(ae.training_step(images(2, 1).cuda())).item()
    finally:
        ae.close()
