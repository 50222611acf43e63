"""Dtype-generic restatement of the autoencoder's decoder (models/encoder/autoencoder.py:23-32) and of the whole
reconstruction loss (:34-37, 48, 55-58) for the decoder tests, on ``F.linear`` / ``F.conv_transpose2d``.

The encoder half is ``encoder_train_ref.encoder_forward_any``; frames come from ``encoder_train_ref.images``.
``per_pixel_decoder`` states the same decoder as the per-pixel GEMMs the kernels run (csrc/decoder.hip): the row and
column orders are spelled out in plain torch so that tests/test_autoencoder_reference.py can hold them against
``F.conv_transpose2d``.
"""
import torch
import torch.nn.functional as F

from encoder_train_ref import KEYS as ENC_KEYS
from encoder_train_ref import encoder_forward_any

DEC_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "6.weight", "6.bias")
_SHAPES = {"0": (9216, 128), "2": (64, 32, 2, 2), "4": (32, 16, 2, 2), "6": (16, 3, 2, 2)}


def make_decoder_state_dict(seed=0):
    """Random-init weights with torch's default initialisers, in the nn.Sequential's own key names.  Linear and
    ConvTranspose2d both draw weight and bias from U(-1/sqrt(fan_in), 1/sqrt(fan_in)) with fan_in = size(1) x the
    receptive field -- for a transposed convolution's (in, out, kH, kW) weight that is out x 4."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in _SHAPES.items():
        fan_in = 1
        for d in shp[1:]:
            fan_in *= d
        bound = 1.0 / fan_in ** 0.5
        n_bias = shp[0] if len(shp) == 2 else shp[1]
        sd[k + ".weight"] = (torch.rand(shp, generator=g) * 2 - 1) * bound
        sd[k + ".bias"] = (torch.rand(n_bias, generator=g) * 2 - 1) * bound
    return sd


def latents(n, seed):
    """Latents at the scale the encoder produces on U[0,1) frames (|z| ~ 0.3), one row of zeros."""
    g = torch.Generator().manual_seed(seed)
    z = 0.3 * torch.randn(n, 128, generator=g)
    z[-1] = 0.0
    return z


def decoder_forward_any(sd, z):
    """(N,128) -> (N,3,96,96) in the dtype of ``z`` / ``sd``."""
    x = F.linear(z, sd["0.weight"], sd["0.bias"]).unflatten(1, (64, 12, 12))
    x = F.relu(F.conv_transpose2d(x, sd["2.weight"], sd["2.bias"], stride=2))
    x = F.relu(F.conv_transpose2d(x, sd["4.weight"], sd["4.bias"], stride=2))
    return torch.sigmoid(F.conv_transpose2d(x, sd["6.weight"], sd["6.bias"], stride=2))


def autoencoder_loss_any(enc_sd, dec_sd, frames):
    recon = decoder_forward_any(dec_sd, encoder_forward_any(enc_sd, frames))
    return torch.mean((recon - frames) ** 2)


def per_pixel_layer(rows, weight, bias):
    """One ConvTranspose2d(cin, cout, 2, stride=2) as the kernels state it: ``rows`` [R][cin] -> [R][4 cout] with column
    kk*cout + co, kk = ky*2 + kx, which read as [4 R][cout] is the next layer's input with row r*4 + kk."""
    cin, cout = weight.shape[:2]
    w = weight.permute(0, 2, 3, 1).reshape(cin, 4 * cout)                  # [ci][kk*cout + co]
    return (rows @ w + bias.repeat(4)).reshape(-1, cout)


def rows_to_nchw(rows, n, levels):
    """[n * 144 * 4^levels][C] rows in the nested order (frame, q, kk1, kk2, ...) -> (n, C, 12 * 2^levels, ...) with the
    pixel at (2^levels qy + ... + 2 ky_{l-1} + ky_l, likewise x)."""
    C = rows.shape[1]
    x = rows.reshape([n, 12, 12] + [2, 2] * levels + [C])                  # n qy qx ky1 kx1 ky2 kx2 ... c
    ys = [1] + [3 + 2 * i for i in range(levels)]
    xs = [2] + [4 + 2 * i for i in range(levels)]
    x = x.permute([0, x.dim() - 1] + ys + xs)
    side = 12 * 2 ** levels
    return x.reshape(n, C, side, side)


def per_pixel_decoder(sd, z, keep=None):
    """``decoder_forward_any`` through the per-pixel GEMMs and row orders of csrc/decoder.hip.  ``keep``: a list that
    receives the three pre-scatter row matrices (after ReLU / before the sigmoid)."""
    n = z.shape[0]
    # the Linear with its rows permuted from Flatten order c*144 + q to q*64 + c: the output is channels-last rows
    w0 = sd["0.weight"].reshape(64, 144, 128).permute(1, 0, 2).reshape(9216, 128)
    b0 = sd["0.bias"].reshape(64, 144).t().reshape(9216)
    h0 = (z @ w0.t() + b0).reshape(n * 144, 64)
    a1 = torch.relu(per_pixel_layer(h0, sd["2.weight"], sd["2.bias"]))     # [n*576][32]
    a2 = torch.relu(per_pixel_layer(a1, sd["4.weight"], sd["4.bias"]))     # [n*2304][16]
    z6 = per_pixel_layer(a2, sd["6.weight"], sd["6.bias"])                 # [n*9216][3]
    if keep is not None:
        keep.extend([a1, a2, z6])
    return torch.sigmoid(rows_to_nchw(z6, n, 3))


def decoder_grads(dec_sd, z, target, dtype=torch.float64, chunk=64, n_total=None):
    """Loss mean((decoder(z) - target)^2) over ALL n frames, its gradients with respect to the decoder's parameters and
    to z, by autograd in ``dtype``, accumulated over chunks of frames.  Returns (loss, {name: gradient}, grad_latent)."""
    n = z.shape[0] if n_total is None else n_total
    params = {k: dec_sd[k].detach().to(dtype).clone().requires_grad_(True) for k in DEC_KEYS}
    loss, gl = 0.0, []
    for i in range(0, z.shape[0], chunk):
        zi = z[i:i + chunk].to(dtype).clone().requires_grad_(True)
        with torch.enable_grad():
            part = ((decoder_forward_any(params, zi) - target[i:i + chunk].to(dtype)) ** 2).sum() / (n * 27648)
            part.backward()
        loss += float(part.detach())
        gl.append(zi.grad.detach())
    return loss, {k: p.grad.detach() for k, p in params.items()}, torch.cat(gl)


def autoencoder_grads(enc_sd, dec_sd, frames, dtype=torch.float64, chunk=64):
    """The reconstruction loss and its gradient for all 16 tensors by autograd in ``dtype``.
    Returns (loss, {enc name: g}, {dec name: g})."""
    n = frames.shape[0]
    pe = {k: enc_sd[k].detach().to(dtype).clone().requires_grad_(True) for k in ENC_KEYS}
    pd = {k: dec_sd[k].detach().to(dtype).clone().requires_grad_(True) for k in DEC_KEYS}
    loss = 0.0
    for i in range(0, n, chunk):
        x = frames[i:i + chunk].to(dtype)
        with torch.enable_grad():
            part = ((decoder_forward_any(pd, encoder_forward_any(pe, x)) - x) ** 2).sum() / (n * 27648)
            part.backward()
        loss += float(part.detach())
    return loss, {k: p.grad.detach() for k, p in pe.items()}, {k: p.grad.detach() for k, p in pd.items()}


# ---- trained-scale data: saturated sigmoid, 8-bit frames with flat patches, dead channels ------------------
TRAINED_CASES = (("trained40", 6), ("trained40", 40), ("trained120", 6), ("trained120", 40))


def case_id(v):
    """pytest id of an ``n`` parameter that is a frame count (today's data) or a (flavour, n) pair of TRAINED_CASES"""
    return str(v) if isinstance(v, int) else f"{v[0]}-{v[1]}"


def trained_decoder_state_dict(seed, k6):
    """``make_decoder_state_dict`` with the last layer scaled by ``k6``: recon from 1e-3 to 0.9996 at 40, from 1e-9 to exactly
    1.0f at 120, where torch's default initialisation keeps it in [0.457, 0.549]."""
    sd = make_decoder_state_dict(seed)
    sd["6.weight"] = sd["6.weight"] * k6
    sd["6.bias"] = sd["6.bias"] * k6
    return sd


def trained_encoder_state_dict(enc_sd):
    """The three convolutions scaled by 3 (latents of std 0.7 instead of 0.026) and a few channels of every ReLU layer dead
    (bias -50: whole columns exactly zero)."""
    sd = {k: v.clone() for k, v in enc_sd.items()}
    for k in ("0.weight", "2.weight", "4.weight"):
        sd[k] = sd[k] * 3
    sd["0.bias"][[2, 9]] = -50.0
    sd["2.bias"][[3, 17, 31]] = -50.0
    sd["4.bias"][[4, 40, 63]] = -50.0
    return sd


def trained_frames(n, seed):
    """8-bit frames k / 255 with a black band that touches the padded border (rows 0-19), a white 20 x 20 patch and a flat grey
    patch."""
    g = torch.Generator().manual_seed(seed)
    x = torch.round(torch.rand(n, 3, 96, 96, generator=g) * 255) / 255
    x[:, :, 0:20, :] = 0.0
    x[:, :, 40:60, 30:50] = 1.0
    x[:, :, 70:90, 60:90] = 128.0 / 255
    return x

