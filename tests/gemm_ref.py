"""Plain float64 CPU reference of ONE implicit-GEMM launch (spdm_op_gemm, include/spdm.h), for tests only.

Built from torch.nn.functional alone -- conv2d(padding=1), linear, group_norm, layer_norm, gelu (erf), max_pool2d(2),
interpolate(bilinear, align_corners=True), cat -- and independent of the package: a pending GroupNorm is evaluated from the
float64 input itself, never from the statistics a kernel wrote.  Tensors are channels-last, as the kernels store them:
a map is (B, H * W, C); a Linear input is (rows, C).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

PRO_NONE, PRO_GN, PRO_GN_GELU, PRO_POOL, PRO_UPCAT = range(5)
EPI_STATS, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_PLAIN = range(5)


def to_nchw(x, H, W):
    return x.reshape(x.shape[0], H, W, x.shape[-1]).permute(0, 3, 1, 2)


def to_cl(x):
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])


def group_norm(x, g, b, cnorm=None):
    """GroupNorm(1, C) of a NCHW map over its first `cnorm` channels (the real ones of padded storage); the padded
    channels carry zero gain and offset, so they come out as zero."""
    c = x.shape[1] if cnorm is None else cnorm
    y = torch.zeros_like(x)
    y[:, :c] = F.group_norm(x[:, :c], 1, g[:c], b[:c], 1e-5)
    return y


def prologue(pro, src, H, W, *, gn=None, skip=None, skip_gn=None, up_C=None, taps=9):
    """The input the contraction sees, NCHW (or (rows, K) for a Linear).  gn / skip_gn: None (nothing pending) or
    (gamma, beta, cnorm) of the GroupNorm pending on src / skip."""
    src = src.double()
    if taps == 1:
        if pro == PRO_NONE:
            return src
        y = F.layer_norm(src, (src.shape[-1],), gn[0].double(), gn[1].double(), 1e-5)
        return F.gelu(y) if pro == PRO_GN_GELU else y
    if pro == PRO_POOL:
        x = to_nchw(src, 2 * H, 2 * W)
        if gn is not None:
            x = group_norm(x, gn[0].double(), gn[1].double(), gn[2])
        return F.max_pool2d(x, 2)
    if pro == PRO_UPCAT or skip is not None:
        if pro == PRO_UPCAT:
            x = to_nchw(src, H // 2, W // 2)
            if gn is not None:
                x = group_norm(x, gn[0].double(), gn[1].double(), gn[2])
            x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        else:                                  # two-source input: src is finished
            x = to_nchw(src, H, W)
        s = to_nchw(skip.double(), H, W)
        if skip_gn is not None:
            s = group_norm(s, skip_gn[0].double(), skip_gn[1].double(), skip_gn[2])
        return torch.cat([x, s], dim=1)
    x = to_nchw(src, H, W)
    if pro in (PRO_GN, PRO_GN_GELU):
        x = group_norm(x, gn[0].double(), gn[1].double(), gn[2])
        if pro == PRO_GN_GELU:
            x = F.gelu(x)
    return x


def contract(x, w, taps):
    """3x3 convolution (padding 1; a 3x1 convolution of a W == 1 map is the same thing) or Linear, no bias."""
    if taps == 1:
        return F.linear(x, w.double())
    return to_cl(F.conv2d(x, w.double(), None, padding=1))


def ref_launch(pro, epi, src, w, H, W, *, taps=9, gn=None, skip=None, skip_gn=None, up_C=None, bias=None, resid=None):
    """(out, bound_scale): the launch's output in float64, and |W| (*) |X~| + |bias| + |resid| -- the same launch on
    absolute values after the prologue, the scale every element's rounding error is measured against."""
    x = prologue(pro, src, H, W, gn=gn, skip=skip, skip_gn=skip_gn, up_C=up_C, taps=taps)
    y = contract(x, w, taps)
    scale = contract(x.abs(), w.abs(), taps)
    if epi != EPI_STATS and epi != EPI_PLAIN:
        y = y + bias.double()
        scale = scale + bias.double().abs()
        if epi == EPI_BIAS_GELU:
            y = F.gelu(y)
        if epi == EPI_BIAS_RESID:
            y = y + resid.double()
            scale = scale + resid.double().abs()
    return y, scale


def floor_terms(pro, src, w, H, W, taps=9, **kw):
    """(|W| (*) 1, 1 (*) |X~|): the launch on a ones input / ones weight -- what the absolute floors of the split format's
    subnormal `lo` half are multiplied by."""
    x = prologue(pro, src, H, W, taps=taps, **kw)
    return contract(torch.ones_like(x), w.abs(), taps), contract(x.abs(), torch.ones_like(w, dtype=torch.float64), taps)


def partials(x, m_tile, n_tile, HW):
    """Raw fp64 GroupNorm partials of a channels-last tensor (B, HW, C) in a producer's slot layout (kernels.h StatsRef):
    slot (mt - first m-tile of the sample) * n_tiles + nt holds {sum, sum of squares} of the sample's rows in m-tile mt,
    channels of n-tile nt.  Returns (buffer (B, slots, 2), slots)."""
    B, _, C = x.shape
    n_tiles = C // n_tile
    slots = ((HW + m_tile - 2) // m_tile + 1) * n_tiles
    out = torch.zeros(B, slots, 2, dtype=torch.float64)
    for b in range(B):
        r0 = b * HW
        first = r0 // m_tile
        for mt in range(first, (r0 + HW - 1) // m_tile + 1):
            lo, hi = max(mt * m_tile, r0) - r0, min((mt + 1) * m_tile, r0 + HW) - r0
            for nt in range(n_tiles):
                blk = x[b, lo:hi, nt * n_tile:(nt + 1) * n_tile].double()
                out[b, (mt - first) * n_tiles + nt] = torch.stack([blk.sum(), (blk * blk).sum()])
    return out, slots


def stats_totals(st, HW, m_tile, n_tiles, B):
    """Per-sample {sum, sum of squares}: the slots a consumer adds (device_utils.h sample_mean_rstd), in its order."""
    out = torch.zeros(B, 2, dtype=torch.float64)
    for b in range(B):
        r0 = b * HW
        n = ((r0 + HW - 1) // m_tile - r0 // m_tile + 1) * n_tiles
        out[b] = st[b, :n].sum(0)
    return out
