"""Torch-CPU restatement of the concat-conditioned U-Net of the reference's ``models/simple_Unet.py`` (``UNet``, the
network ``Diffusion_DDPM(model='UNet')`` builds), written from its semantics as a functional evaluation of a
``state_dict``.  Test infrastructure only: the GPU tests compare libspdm_hip.so against it where no fixture covers a
shape, and ``tests/test_simple_unet.py`` pins it against the fixtures recorded from the reference module itself
(tools/make_golden_simple.py).  Eval semantics: the positional encoding's dropout is off.

    x -> pad_to(x, 8) -> input_conv = DC(1, 16)
      -> down1..3: MaxPool2d(2), DC(Cin, Cin, residual), DC(Cin, Cout), + Linear(SiLU(pe[t])), cat 32 x Linear(SiLU(cond))
      -> up1..3:   Upsample(x2, bilinear, align_corners=True), cat skip, DC(residual), DC, + emb, cat 32 cond channels
      -> outc (1x1 conv, bias) -> unpad
    DC(x) = GELU(GN(conv2(GELU(GN(conv1(x))))) [+ x])   (one GroupNorm(1, C) module for both convolutions)
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def _t(sd, name):
    v = sd[name]
    return v if isinstance(v, torch.Tensor) else torch.from_numpy(v)


def pad_to_8(x):
    """Zero-pad H and W up to a multiple of 8, the smaller half of the padding first (pad_to, simple_Unet.py:13-33)."""
    h, w = x.shape[-2:]
    ph = (-h) % 8
    pw = (-w) % 8
    pads = (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)
    return F.pad(x, pads), pads


def unpad(x, pads):
    lw, uw, lh, uh = pads
    return x[..., lh:x.shape[-2] - uh, lw:x.shape[-1] - uw]


def double_conv(sd, p, x, residual=False):
    g, b = _t(sd, f"{p}.norm.weight"), _t(sd, f"{p}.norm.bias")
    h = F.conv2d(x, _t(sd, f"{p}.first.weight"), padding=1)
    h = F.gelu(F.group_norm(h, 1, g, b))
    h = F.conv2d(h, _t(sd, f"{p}.second.weight"), padding=1)
    h = F.group_norm(h, 1, g, b)
    return F.gelu(h + x) if residual else F.gelu(h)


def _block_tail(sd, p, x, pe_t, cond):
    emb = F.linear(F.silu(pe_t), _t(sd, f"{p}.emb_layer.1.weight"), _t(sd, f"{p}.emb_layer.1.bias"))   # (1|B, C)
    x = x + emb[:, :, None, None]
    c = F.linear(F.silu(cond.reshape(cond.shape[0], -1)), _t(sd, f"{p}.cond_emb_layer.1.weight"),
                 _t(sd, f"{p}.cond_emb_layer.1.bias"))                                                  # (B, 32)
    return torch.cat([x, c[:, :, None, None].expand(-1, -1, x.shape[-2], x.shape[-1])], dim=1)


def down(sd, p, x, pe_t, cond):
    x = F.max_pool2d(x, 2)
    x = double_conv(sd, f"{p}.doubleConv1", x, residual=True)
    x = double_conv(sd, f"{p}.doubleConv2", x)
    return _block_tail(sd, p, x, pe_t, cond)


def up(sd, p, x, skip, pe_t, cond):
    x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    x = torch.cat([x, skip], dim=1)
    x = double_conv(sd, f"{p}.doubleConv1", x, residual=True)
    x = double_conv(sd, f"{p}.doubleConv2", x)
    return _block_tail(sd, p, x, pe_t, cond)


@torch.no_grad()
def simple_unet_forward(sd, x, t, y):
    """eps = UNet(x, t, y) for x (B,1,H,D), t (1,) or (B,) int, y (B,1,obs_h,obs_dim) (required: the reference's channel
    counts only match with conditioning)."""
    if y is None:
        raise ValueError("simple_Unet.UNet needs its conditioning y")
    dt = torch.float64 if torch.as_tensor(x).dtype == torch.float64 else torch.float32   # (float64: high-precision evaluation)
    x = torch.as_tensor(x, dtype=dt)
    y = torch.as_tensor(y, dtype=dt)
    t = torch.as_tensor(t, dtype=torch.int64).reshape(-1)
    xp, pads = pad_to_8(x)
    pe_t = _t(sd, "pos_encoding.pos_encoding")[t]                  # (1|B, time_dim)
    x1 = double_conv(sd, "input_conv", xp)
    x2 = down(sd, "down1", x1, pe_t, y)
    x3 = down(sd, "down2", x2, pe_t, y)
    x4 = down(sd, "down3", x3, pe_t, y)
    h = up(sd, "up1", x4, x3, pe_t, y)
    h = up(sd, "up2", h, x2, pe_t, y)
    h = up(sd, "up3", h, x1, pe_t, y)
    out = F.conv2d(h, _t(sd, "outc.weight"), _t(sd, "outc.bias"))
    return unpad(out, pads)
