"""CPU checks of the float64 launch reference (tests/gemm_ref.py) and of the data the GPU launch tests feed it
(tests/test_gpu_gemm_fp64.py): the reference agrees with the oracle, and every plausible kernel defect moves the
reference by at least 100 x the tolerance on the compared elements -- a generator that cannot tell a defect apart does
not test it."""
import torch
import torch.nn.functional as F

from gemm_ref import (EPI_BIAS, EPI_BIAS_RESID, EPI_STATS, PRO_GN, PRO_GN_GELU, PRO_NONE, PRO_POOL, PRO_UPCAT,
                      floor_terms, group_norm, partials, ref_launch, stats_totals, to_cl, to_nchw)
from oracle.unet_film_ref import double_conv
from test_gpu_gemm_fp64 import TAU_SPLIT, FLOOR_W, FLOOR_X, activations, gains, weights

B, H, W, C = 6, 8, 4, 64
HW = H * W


def bound(pro, src, w, h, wd, scale, **kw):
    fl = floor_terms(pro, src, w, h, wd, **kw)
    return TAU_SPLIT * scale + FLOOR_X * fl[0] + FLOOR_W * fl[1]


def worst(a, b, bnd):
    return float(((a - b).abs() / bnd).max())


def test_chain_matches_oracle_double_conv():
    x = activations(B, HW, C, 1, "edges")
    g, b = gains(C, 2, "edges")
    w1, w2 = weights(C, C, 9, 3), weights(C, C, 9, 4)
    y1, _ = ref_launch(PRO_NONE, EPI_STATS, x, w1, H, W)
    y2, _ = ref_launch(PRO_GN_GELU, EPI_STATS, y1, w2, H, W, gn=(g, b, None))
    got = to_cl(group_norm(to_nchw(y2, H, W), g.double(), b.double()))
    sd = {"p.first.weight": w1.double(), "p.second.weight": w2.double(), "p.norm.weight": g.double(), "p.norm.bias": b.double()}
    want = to_cl(double_conv(sd, "p", to_nchw(x.double(), H, W)))
    assert float((got - want).abs().max()) <= 1e-12


def test_pool_and_upsample_read_through_match_oracle_steps():
    """The oracle's DownSample / UpSample input steps (max_pool2d(2); bilinear x2 align_corners=True + cat), fed to the same
    convolution."""
    w = weights(C, C, 9, 5)
    x = activations(B, 4 * HW, C, 6, "unit")
    got, _ = ref_launch(PRO_POOL, EPI_STATS, x, w, H, W)
    want = to_cl(F.conv2d(F.max_pool2d(to_nchw(x.double(), 2 * H, 2 * W), 2), w.double(), padding=1))
    assert float((got - want).abs().max()) <= 1e-12
    up = activations(B, HW // 4, 32, 7, "unit")
    skip = activations(B, HW, 32, 8, "unit")
    got, _ = ref_launch(PRO_UPCAT, EPI_STATS, up, w, H, W, skip=skip, up_C=32)
    u = F.interpolate(to_nchw(up.double(), H // 2, W // 2), scale_factor=2, mode="bilinear", align_corners=True)
    want = to_cl(F.conv2d(torch.cat([u, to_nchw(skip.double(), H, W)], 1), w.double(), padding=1))
    assert float((got - want).abs().max()) <= 1e-12


def test_partials_layout_totals():
    x = activations(5, 48, 64, 9, "edges")
    st, slots = partials(x, 64, 32, 48)
    tot = stats_totals(st, 48, 64, 2, 5)
    assert torch.allclose(tot[:, 0], x.double().sum((1, 2)), rtol=1e-12, atol=1e-9)
    assert torch.allclose(tot[:, 1], (x.double() ** 2).sum((1, 2)), rtol=1e-12)


def test_defects_are_visible():
    w = weights(C, C, 9, 11)
    g, b = gains(C, 12, "edges")
    gn = (g, b, None)

    # affine after the max instead of before (negative gains make the two differ)
    x = activations(B, 4 * HW, C, 13, "edges")
    want, scale = ref_launch(PRO_POOL, EPI_STATS, x, w, H, W, gn=gn)
    bnd = bound(PRO_POOL, x, w, H, W, scale, gn=gn)
    xn = to_nchw(x.double(), 2 * H, 2 * W)
    mean = xn.mean((1, 2, 3), keepdim=True)
    var = xn.var((1, 2, 3), unbiased=False, keepdim=True)
    pooled = F.max_pool2d(xn, 2)
    late = (pooled - mean) / (var + 1e-5).sqrt() * g.double()[None, :, None, None] + b.double()[None, :, None, None]
    bad = to_cl(F.conv2d(late, w.double(), padding=1))
    assert worst(bad, want, bnd) >= 100, "affine after max"

    # beta dropped
    x = activations(B, HW, C, 14, "edges")
    want, scale = ref_launch(PRO_GN_GELU, EPI_STATS, x, w, H, W, gn=gn)
    bnd = bound(PRO_GN_GELU, x, w, H, W, scale, gn=gn)
    bad, _ = ref_launch(PRO_GN_GELU, EPI_STATS, x, w, H, W, gn=(g, torch.zeros_like(b), None))
    assert worst(bad, want, bnd) >= 100, "beta dropped"

    # one slot of the partials missing (the consumer's statistics lose a tile)
    st, slots = partials(x, 16, 32, HW)
    st_bad = st.clone()
    st_bad[:, 1] = 0.0
    tot = stats_totals(st_bad, HW, 16, 2, B)
    n = HW * C
    m = tot[:, 0] / n
    v = tot[:, 1] / n - m * m
    xn = to_nchw(x.double(), H, W)
    y = (xn - m[:, None, None, None]) / (v[:, None, None, None] + 1e-5).sqrt() * g.double()[None, :, None, None] + b.double()[None, :, None, None]
    bad = to_cl(F.conv2d(F.gelu(y), w.double(), padding=1))
    assert worst(bad, want, bnd) >= 100, "slot missing"

    # the ragged last tile's rows zeroed (m_tile 256 over HW = 32 rows: the last 2 samples of 6)
    assert worst(torch.zeros_like(want[-2:]), want[-2:], bnd[-2:]) >= 100, "ragged tile zeroed"

    # residual dropped
    xl = activations(B * HW, 1, C, 15, "edges").reshape(B * HW, C)
    wl = weights(C, C, 1, 16)
    bias = torch.rand(C, dtype=torch.float64).float()
    resid = torch.rand(B * HW, C, dtype=torch.float64).float() * 2 - 1
    want, scale = ref_launch(PRO_NONE, EPI_BIAS_RESID, xl, wl, 1, 1, taps=1, bias=bias, resid=resid)
    bad, _ = ref_launch(PRO_NONE, EPI_BIAS, xl, wl, 1, 1, taps=1, bias=bias)
    assert worst(bad, want, TAU_SPLIT * scale) >= 100, "residual dropped"

    # align_corners=False
    up = activations(B, HW // 4, 32, 17, "edges")
    skip = activations(B, HW, 32, 18, "edges")
    want, scale = ref_launch(PRO_UPCAT, EPI_STATS, up, w, H, W, skip=skip, up_C=32)
    bnd = bound(PRO_UPCAT, up, w, H, W, scale, skip=skip, up_C=32)
    u = F.interpolate(to_nchw(up.double(), H // 2, W // 2), scale_factor=2, mode="bilinear", align_corners=False)
    bad = to_cl(F.conv2d(torch.cat([u, to_nchw(skip.double(), H, W)], 1), w.double(), padding=1))
    assert worst(bad, want, bnd) >= 100, "align_corners=False"

    # statistics over the padded width instead of the real channel count
    k = 48
    x = activations(B, HW, C, 19, "edges", cnorm=k)
    gp, bp = gains(C, 20, "edges", cnorm=k)
    wp = weights(C, C, 9, 21, kreal=k, nreal=40)
    want, scale = ref_launch(PRO_GN_GELU, EPI_STATS, x, wp, H, W, gn=(gp, bp, k))
    bnd = bound(PRO_GN_GELU, x, wp, H, W, scale, gn=(gp, bp, k))
    bad, _ = ref_launch(PRO_GN_GELU, EPI_STATS, x, wp, H, W, gn=(gp, bp, C))
    assert worst(bad, want, bnd) >= 100, "padded-width statistics"
