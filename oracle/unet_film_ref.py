"""ORACLE (test infrastructure only -- never imported by the product path).

CPU restatement, in plain torch-CPU fp32 functional ops, of the reference's
FiLM-conditioned U-Net noise predictor ``UNet_Film.forward``
(``/root/reference/models/Unet_FiLmLayer.py:277-312``) and of the no-attention
variant (``models/Unet_FiLmLayer_noAttention.py:277-300``).  Only ``tests/``,
``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import
this file; the product (``state_policy_diffusionmodel_amd``) must not.

Pinning: ``tools/make_golden.py`` (run in the build container, where
``/root/reference`` exists) imports the reference module, loads the SAME
generated ``state_dict`` into it with ``strict=True``, runs it on seeded inputs
and commits inputs + outputs under ``tests/golden/``;
``tests/test_oracle.py`` checks this restatement against those vectors, and
``tests/test_oracle_vs_reference.py`` against the reference's recorded
state_dict inventory and forward outputs (``ref_inventory.json``, ``refpin_*.npz``).

The restatement is deliberately NOT a module tree: it is a flat function over
a name -> tensor dict, written from the reference's behaviour, one helper per
reference class, each citing the lines it follows.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F


def _as_torch(sd) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in sd.items():
        out[k] = v if isinstance(v, torch.Tensor) else torch.from_numpy(v)
    return out


def pad_amounts(h: int, w: int, stride: int = 8):
    """(lw, uw, lh, uh) exactly as ``pad_to`` computes them
    (models/Unet_FiLmLayer.py:15-28): pad up to the next multiple of
    ``stride``; the lower pad is ``int(extra / 2)``, the upper pad the rest."""
    new_h = h + stride - h % stride if h % stride > 0 else h
    new_w = w + stride - w % stride if w % stride > 0 else w
    lh = int((new_h - h) / 2)
    uh = int(new_h - h) - lh
    lw = int((new_w - w) / 2)
    uw = int(new_w - w) - lw
    return lw, uw, lh, uh


def sinusoid_table(t: torch.Tensor, channels: int = 256, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``UNet_Film.pos_encoding`` (models/Unet_FiLmLayer.py:266-274) applied to
    ``t.unsqueeze(-1).float()`` (``:281``): [sin(t*f) || cos(t*f)] with
    f_i = 1 / 10000**(2i/channels); halves concatenated, not interleaved.
    ``dtype``: float32 as the reference; float64 for a high-precision evaluation of the same network."""
    t = t.reshape(-1, 1).to(dtype)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, channels, 2, dtype=dtype) / channels))
    arg = t.repeat(1, channels // 2) * inv_freq
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)


def double_conv(sd, p: str, x: torch.Tensor) -> torch.Tensor:
    """``DoubleConvolution.forward`` (models/Unet_FiLmLayer.py:108-115):
    conv3x3(no bias) -> GroupNorm(1, C) -> GELU(erf) -> conv3x3 -> the SAME
    GroupNorm affine again; no residual, no activation at the end."""
    g, b = sd[f"{p}.norm.weight"], sd[f"{p}.norm.bias"]
    x = F.conv2d(x, sd[f"{p}.first.weight"], None, padding=1)
    x = F.gelu(F.group_norm(x, 1, g, b, 1e-5))
    x = F.conv2d(x, sd[f"{p}.second.weight"], None, padding=1)
    return F.group_norm(x, 1, g, b, 1e-5)


def _time_and_film(sd, p: str, x: torch.Tensor, temb: torch.Tensor,
                   cond: Optional[torch.Tensor]) -> torch.Tensor:
    """Tail shared by DownSample/UpSample (models/Unet_FiLmLayer.py:165-177 and
    :222-234): x + Linear(SiLU(temb)) broadcast over H,W, then FiLM
    ``scale * x + bias`` with [scale | bias] = Linear(Mish(flatten(cond)))."""
    e = F.linear(F.silu(temb), sd[f"{p}.emb_layer.1.weight"], sd[f"{p}.emb_layer.1.bias"])
    x = x + e[:, :, None, None]
    if cond is not None:
        c = x.shape[1]
        f = F.linear(F.mish(cond).flatten(1), sd[f"{p}.cond_encoder.2.weight"],
                     sd[f"{p}.cond_encoder.2.bias"])
        scale, bias = f[:, :c], f[:, c:]
        x = scale[:, :, None, None] * x + bias[:, :, None, None]
    return x


def down_block(sd, p, x, temb, cond):
    """``DownSample.forward`` (models/Unet_FiLmLayer.py:158-179)."""
    x = F.max_pool2d(x, 2)
    x = double_conv(sd, f"{p}.doubleConv1", x)
    x = double_conv(sd, f"{p}.doubleConv2", x)
    return _time_and_film(sd, p, x, temb, cond)


def up_block(sd, p, x, skip, temb, cond):
    """``UpSample.forward`` (models/Unet_FiLmLayer.py:216-237): bilinear x2
    with align_corners=True, concat [upsampled, skip] on channels."""
    x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    x = torch.cat([x, skip], dim=1)
    x = double_conv(sd, f"{p}.doubleConv1", x)
    x = double_conv(sd, f"{p}.doubleConv2", x)
    return _time_and_film(sd, p, x, temb, cond)


def self_attention(sd, p: str, x: torch.Tensor, heads: int = 4) -> torch.Tensor:
    """``SelfAttention.forward`` (models/Unet_FiLmLayer.py:71-82) with
    ``nn.MultiheadAttention(C, 4, batch_first=True)`` written out: tokens are
    the H*W positions; LN -> packed in-proj -> per-head softmax(q k^T / sqrt d) v
    -> out-proj -> + tokens -> LN -> Linear -> GELU -> Linear -> + ."""
    b, c, h, w = x.shape
    tok = x.reshape(b, c, h * w).transpose(1, 2)                      # (B, L, C)
    ln = F.layer_norm(tok, (c,), sd[f"{p}.ln.weight"], sd[f"{p}.ln.bias"], 1e-5)
    qkv = F.linear(ln, sd[f"{p}.attention.in_proj_weight"], sd[f"{p}.attention.in_proj_bias"])
    q, k, v = qkv.split(c, dim=-1)
    d = c // heads

    def split_heads(z):
        return z.reshape(b, h * w, heads, d).permute(0, 2, 1, 3)       # (B, heads, L, d)

    q, k, v = split_heads(q), split_heads(k), split_heads(v)
    att = torch.softmax((q * (1.0 / math.sqrt(d))) @ k.transpose(-1, -2), dim=-1)
    o = (att @ v).permute(0, 2, 1, 3).reshape(b, h * w, c)
    o = F.linear(o, sd[f"{p}.attention.out_proj.weight"], sd[f"{p}.attention.out_proj.bias"])
    a = o + tok
    f = F.layer_norm(a, (c,), sd[f"{p}.ff_self.0.weight"], sd[f"{p}.ff_self.0.bias"], 1e-5)
    f = F.linear(f, sd[f"{p}.ff_self.1.weight"], sd[f"{p}.ff_self.1.bias"])
    f = F.linear(F.gelu(f), sd[f"{p}.ff_self.3.weight"], sd[f"{p}.ff_self.3.bias"])
    out = f + a
    return out.transpose(1, 2).reshape(b, c, h, w)


@torch.no_grad()
def unet_film_forward(sd, x: torch.Tensor, t: torch.Tensor, y: Optional[torch.Tensor],
                      attention: bool = True, time_dim: int = 256,
                      taps: Optional[dict] = None) -> torch.Tensor:
    """``UNet_Film.forward(x, t, y)`` (models/Unet_FiLmLayer.py:277-312).

    x: (B,1,H,D) f32;  t: (1,) or (B,) integer;  y: (B,1,obs_h,obs_dim) f32 or None.
    Returns eps (B,1,H,D).  ``taps`` (optional dict) receives the named
    intermediates in NCHW for block-level tests."""
    sd = _as_torch(sd)
    dt = torch.float64 if x.dtype == torch.float64 else torch.float32      # (float64: a high-precision evaluation)
    x = x.to(dt)
    temb = sinusoid_table(t, time_dim, dt)
    lw, uw, lh, uh = pad_amounts(x.shape[-2], x.shape[-1], 8)
    xp = F.pad(x, (lw, uw, lh, uh), "constant", 0.0)

    def sa(name, z):
        return self_attention(sd, name, z) if attention else z

    def tap(name, z):
        if taps is not None:
            taps[name] = z.clone()
        return z

    x1 = tap("x1", double_conv(sd, "inc", xp))
    x2 = tap("d1", down_block(sd, "down1", x1, temb, y))
    x2 = tap("x2", sa("sa1", x2))
    x3 = tap("d2", down_block(sd, "down2", x2, temb, y))
    x3 = tap("x3", sa("sa2", x3))
    x4 = tap("d3", down_block(sd, "down3", x3, temb, y))
    x4 = tap("x4", sa("sa3", x4))
    x5 = double_conv(sd, "bot1", x4)
    x5 = double_conv(sd, "bot2", x5)
    x5 = tap("x5", double_conv(sd, "bot3", x5))
    u = tap("u1", up_block(sd, "up1", x5, x3, temb, y))
    u = tap("a4", sa("sa4", u))
    u = tap("u2", up_block(sd, "up2", u, x2, temb, y))
    u = tap("a5", sa("sa5", u))
    u = tap("u3", up_block(sd, "up3", u, x1, temb, y))
    u = tap("a6", sa("sa6", u))
    out = F.conv2d(u, sd["outc.weight"], sd["outc.bias"])
    hp, wp = out.shape[-2], out.shape[-1]
    out = out[:, :, lh:hp - uh, lw:wp - uw]                              # unpad, :36-41
    return out.contiguous()
