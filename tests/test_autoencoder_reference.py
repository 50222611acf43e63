"""The decoder tests' reference against torch itself, without a GPU: the dtype-generic restatement
(tests/autoencoder_ref.py) equals the nn.Sequential of models/encoder/autoencoder.py:23-32 bit for bit in fp32; the
per-pixel-GEMM row / column orders the kernels use (csrc/decoder.hip) reproduce F.conv_transpose2d; fp32 autograd of the
whole autoencoder stays within the training bound of float64 autograd on the tests' inputs (measured here: worst tensor
4.2e-6 over n = 1, 6, 40, 130 on these seeds); and the checkpoint key mapping round trips."""
import pytest
import torch
import torch.nn.functional as F

from autoencoder_ref import (DEC_KEYS, TRAINED_CASES, autoencoder_grads, case_id, decoder_forward_any, decoder_grads, latents,
                             make_decoder_state_dict, per_pixel_decoder, per_pixel_layer, rows_to_nchw,
                             trained_decoder_state_dict, trained_encoder_state_dict, trained_frames)
from encoder_train_ref import KEYS as ENC_KEYS
from encoder_train_ref import encoder_grads, images
from oracle.encoder_ref import make_encoder_state_dict

BOUND = 1e-4


def _sequential(sd):
    nn = torch.nn
    dec = nn.Sequential(nn.Linear(128, 64 * 12 * 12), nn.Unflatten(1, (64, 12, 12)), nn.ConvTranspose2d(64, 32, 2, stride=2),
                        nn.ReLU(), nn.ConvTranspose2d(32, 16, 2, stride=2), nn.ReLU(), nn.ConvTranspose2d(16, 3, 2, stride=2),
                        nn.Sigmoid())
    dec.load_state_dict(sd, strict=True)
    return dec.eval()


def test_restatement_equals_the_sequential_bit_for_bit_in_fp32():
    sd = make_decoder_state_dict(3)
    z = latents(5, 1)
    with torch.no_grad():
        assert torch.equal(decoder_forward_any(sd, z), _sequential(sd)(z))


def test_state_dict_maker_has_torch_default_bounds():
    sd = make_decoder_state_dict(1)
    assert tuple(sd) == DEC_KEYS
    for k, fan_in in (("0", 128), ("2", 128), ("4", 64), ("6", 12)):
        b = 1.0 / fan_in ** 0.5
        for t in (sd[k + ".weight"], sd[k + ".bias"]):
            assert float(t.abs().max()) <= b
        assert float(sd[k + ".weight"].abs().max()) > 0.9 * b


@pytest.mark.parametrize("cin,cout,levels", [(64, 32, 1), (32, 16, 2), (16, 3, 3)])
def test_per_pixel_gemm_orders_reproduce_conv_transpose2d(cin, cout, levels):
    """Rows (frame, q, kk1, ..) x columns kk*cout + co, read as four times as many rows of cout, are the transposed
    convolution's output with the pixel at (2 y + ky, 2 x + kx) -- float64, so only the order can differ."""
    g = torch.Generator().manual_seed(cin)
    n = 2
    rows = torch.randn(n * 144 * 4 ** (levels - 1), cin, generator=g, dtype=torch.float64)
    w = torch.randn(cin, cout, 2, 2, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(rows_to_nchw(rows, n, levels - 1), w, b, stride=2)
    got = rows_to_nchw(per_pixel_layer(rows, w, b), n, levels)
    assert got.shape == want.shape == (n, cout, 12 * 2 ** levels, 12 * 2 ** levels)
    assert float((got - want).abs().max()) <= 1e-12


def test_per_pixel_decoder_equals_the_restatement():
    sd = {k: v.double() for k, v in make_decoder_state_dict(4).items()}
    z = latents(3, 2).double()
    keep = []
    got = per_pixel_decoder(sd, z, keep)
    assert float((got - decoder_forward_any(sd, z)).abs().max()) <= 1e-12
    assert [tuple(t.shape) for t in keep] == [(3 * 576, 32), (3 * 2304, 16), (3 * 9216, 3)]
    # the last layer's scatter: row ((q*4 + kk1)*4 + kk2)*4 + kk3 of frame 0 is pixel (8qy + 4ky1 + 2ky2 + ky3, ...)
    q, kk1, kk2, kk3 = 17, 2, 1, 3
    y = 8 * (q // 12) + 4 * (kk1 >> 1) + 2 * (kk2 >> 1) + (kk3 >> 1)
    x = 8 * (q % 12) + 4 * (kk1 & 1) + 2 * (kk2 & 1) + (kk3 & 1)
    assert torch.equal(torch.sigmoid(keep[2][((q * 4 + kk1) * 4 + kk2) * 4 + kk3]), got[0, :, y, x])


@pytest.mark.parametrize("n", [1, 6, 40, 130, *TRAINED_CASES], ids=case_id)
def test_fp32_autograd_is_within_the_bound_of_float64(n):
    """Guards the inputs: if torch's own fp32 autograd could not hold the bound on these frames and weights (a ReLU
    unit rounding to the other side of its kink carries a whole unit's gradient), no fp32 kernel could.  The (flavour, n)
    cases are the trained-scale data of tests/test_gpu_decoder.py (measured here: worst tensor 5.8e-6, loss 9e-8)."""
    enc_sd, dec_sd = make_encoder_state_dict(5), make_decoder_state_dict(6)
    if isinstance(n, int):
        x = images(n, 100 + n)
    else:
        enc_sd, dec_sd = trained_encoder_state_dict(enc_sd), trained_decoder_state_dict(6, int(n[0][7:]))
        x, n = trained_frames(n[1], 100 + n[1]), n[1]
    l64, e64, d64 = autoencoder_grads(enc_sd, dec_sd, x)
    l32, e32, d32 = autoencoder_grads(enc_sd, dec_sd, x, dtype=torch.float32)
    assert abs(l32 - l64) <= 1e-6 * l64
    worst = {}
    for tag, a, b, keys in (("enc/", e32, e64, ENC_KEYS), ("dec/", d32, d64, DEC_KEYS)):
        for k in keys:
            worst[tag + k] = float((a[k].double() - b[k]).norm() / b[k].norm())
    print(f"\nAUTOENCODER fp32 vs float64 n={n}: worst {max(worst.values()):.2e} ({max(worst, key=worst.get)})")
    assert max(worst.values()) <= BOUND, worst


@pytest.mark.parametrize("case", TRAINED_CASES, ids=case_id)
def test_fp32_autograd_of_the_decoder_alone_is_within_the_bound_on_trained_scale_data(case):
    """The decoder cases of tests/test_gpu_decoder.py: latents against 8-bit frames (measured: worst tensor 8.3e-6, loss 1.4e-7).
    Targets equal to the reconstruction rounded to 8 bits are NOT usable at this level: recon - target cancels, the gradient is
    what float32 leaves of it, and torch's own fp32 autograd misses float64 by 1.0e-4 to 1.3e-4; tests/frame_ops_ref.py holds
    that data per launch instead."""
    n = case[1]
    sd = trained_decoder_state_dict(6, int(case[0][7:]))
    z, tgt = latents(n, 10 + n), trained_frames(n, 200 + n)
    l64, g64, gl64 = decoder_grads(sd, z, tgt)
    l32, g32, gl32 = decoder_grads(sd, z, tgt, dtype=torch.float32)
    assert abs(l32 - l64) <= 1e-6 * l64
    worst = {k: float((g32[k].double() - g64[k]).norm() / g64[k].norm()) for k in DEC_KEYS}
    worst["grad_latent"] = float((gl32.double() - gl64).norm() / gl64.norm())
    assert max(worst.values()) <= BOUND, worst
    with torch.no_grad():                                                      # the data do what they are for
        recon = decoder_forward_any(sd, z)
    assert float(recon.min()) < 2e-3 and float(recon.max()) > 0.999


@pytest.mark.parametrize("n", [6, 40])
def test_fp32_autograd_of_the_encoder_alone_is_within_the_bound_on_trained_scale_data(n):
    """The ("trained", n) cases of tests/test_gpu_encoder_train.py (measured: worst tensor 2.3e-6)."""
    sd, x = trained_encoder_state_dict(make_encoder_state_dict(5)), trained_frames(n, 100 + n)
    gl = torch.randn(n, 128, generator=torch.Generator().manual_seed(n)) / (n * 128)
    lat, g64 = encoder_grads(sd, x, gl)
    _, g32 = encoder_grads(sd, x, gl, dtype=torch.float32)
    assert max(float((g32[k].double() - g64[k]).norm() / g64[k].norm()) for k in ENC_KEYS) <= BOUND
    assert 0.3 < float(lat.std()) < 3.0                                        # latents of order 1, not 0.026


def test_checkpoint_key_mapping_round_trips():
    from state_policy_diffusionmodel_amd.autoencoder import DECODER_KEYS, DECODER_SHAPES, decoder_state_dict_from
    from state_policy_diffusionmodel_amd.vision import encoder_state_dict_from
    assert DECODER_KEYS == DEC_KEYS
    enc_sd, dec_sd = make_encoder_state_dict(1), make_decoder_state_dict(2)
    assert {k: tuple(v.shape) for k, v in dec_sd.items()} == DECODER_SHAPES
    for pre in ("decoder.", "model.decoder.", ""):
        got = decoder_state_dict_from({pre + k: v for k, v in dec_sd.items()})
        assert tuple(got) == DEC_KEYS and all(got[k] is dec_sd[k] for k in DEC_KEYS)
    assert decoder_state_dict_from({k: v for k, v in dec_sd.items() if k != "6.bias"}) is None
    assert decoder_state_dict_from({"encoder." + k: v for k, v in enc_sd.items()}) is None
    # a Lightning checkpoint of the reference's autoencoder registers both halves twice (model.* and the aliases)
    ckpt = {}
    for pre in ("model.", ""):
        ckpt.update({f"{pre}encoder.{k}": v for k, v in enc_sd.items()})
        ckpt.update({f"{pre}decoder.{k}": v for k, v in dec_sd.items()})
    assert all(decoder_state_dict_from(ckpt)[k] is dec_sd[k] for k in DEC_KEYS)
    assert all(encoder_state_dict_from(ckpt)[k] is enc_sd[k] for k in ENC_KEYS)
    only_model = {k: v for k, v in ckpt.items() if k.startswith("model.")}
    assert all(decoder_state_dict_from(only_model)[k] is dec_sd[k] for k in DEC_KEYS)
