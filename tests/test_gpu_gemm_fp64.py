"""Every implicit-GEMM route of launch_gemm, one launch at a time (spdm_op_gemm), against a plain float64 CPU reference
(tests/gemm_ref.py) on data the test controls.

Tolerance, per element:  |got - want| <= TAU * (|W| (*) |X~| + |bias| + |resid|) + FLOOR_X * (|W| (*) 1) + FLOOR_W * (1 (*) |X~|)
where (*) is the same launch evaluated in float64 after the prologue.  FLOOR_X / FLOOR_W are the absolute floors of the
split format's `lo` half where it is an fp16 subnormal; the exact fp32 path has none.  Every case asserts
the kernel it is meant to hit.  Shapes with many rows compare a fixed subset of samples (first, last, both sides of every
tile boundary inside a sample, the ragged last tile, 8 seeded random ones); the GroupNorm totals are checked for all.

TAU was set from the first measured run (MI355X; the data are seeded and the kernels deterministic).  Worst measured ratio
of error to bound per route and data flavour ('edges' = offsets / zero sample / mixed gains with pending GroupNorms;
'big' = |activation| up to 3000 and |weight| up to 400, raw inputs; sweep = 2^-12 .. 2^8):
    route                                      edges   big    sweep
    conv3x3_wide_kernel (incl. published)      0.37    0.04   0.09
    conv_reg64_kernel                          0.65    0.05   0.11
    conv_skinny_kernel (incl. fused sources)   0.40    0.02   0.06
    conv_gemm_kernel 3x3, split                0.37    0.03   0.07
    conv_gemm_kernel, exact fp32 (TAU_EXACT)   0.44    0.14   -
    split-K + splitk_combine_kernel            0.34    0.02   0.07
    Linear, split / exact                      0.04 / 0.11    0.04 / 0.13   0.16
    Linear -> row_stats -> LayerNorm Linear    0.07
    simple-UNet padded channels                0.48
The worst cases are the GroupNorm prologues on per-sample offsets of 50 (the fp32 (x - mean) of the prologue); the chained
DoubleConvolution is within 1.7e-6 (B = 2) and 4.8e-6 (B = 1024) of the float64 oracle.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from gemm_ref import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_PLAIN, EPI_STATS, PRO_GN, PRO_GN_GELU, PRO_NONE,
                      PRO_POOL, PRO_UPCAT, floor_terms, partials, ref_launch, stats_totals)

pytestmark = pytest.mark.gpu

TAU_SPLIT = 4e-6
TAU_EXACT = 2e-6
FLOOR_X = 2.0 ** -29      # activation: 2^-25 (half the fp16 subnormal spacing) of the x 2^4 pre-scaled lo, scaled back
FLOOR_W = 2.0 ** -32      # weight: the same under the x 2^7 pre-scale
GEMM, SKINNY, REG, WIDE = 0, 1, 2, 3
PLAIN, W2, WP4, WP8, PIPE = 0, 1, 2, 3, 4


def _lib():
    from state_policy_diffusionmodel_amd import _lib as L
    return L, L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def op_gemm(B, H, W, K, N, taps, split, pro, epi, src, w, *, skip=None, up_C=0, src_st=None, gamma=None, beta=None,
            skip_st=None, skip_gamma=None, skip_beta=None, bias=None, resid=None, row_stats=False, check=True):
    """Run one launch; src_st / skip_st: (partials (B, slots, 2) fp64, slots, m_tile, n_tiles, cnorm)."""
    L, lib = _lib()
    HW = H * W
    M = B * HW
    dev = lambda t, dt=torch.float32: None if t is None else t.to(dt).contiguous().cuda()
    a = L.SpdmOpGemmArgs()
    a.B, a.H, a.W, a.K, a.N, a.taps, a.split, a.pro, a.epi = B, H, W, K, N, taps, split, pro, epi
    keep = []
    d_src = dev(src)
    keep.append(d_src)
    a.d_src, a.src_ld = _p(d_src), d_src.shape[-1]
    if skip is not None:
        d_skip = dev(skip)
        keep.append(d_skip)
        a.d_skip, a.skip_ld, a.up_C = _p(d_skip), d_skip.shape[-1], up_C
    wh = w.float().contiguous().numpy()
    a.h_weight = wh.ctypes.data_as(ctypes.c_void_p)
    if src_st is not None:
        t = dev(src_st[0], torch.float64)
        keep += [t]
        a.d_src_stats, a.src_slots, a.src_m_tile, a.src_n_tiles, a.src_cnorm = _p(t), *src_st[1:]
    for name, v in (("d_gamma", gamma), ("d_beta", beta), ("d_skip_gamma", skip_gamma), ("d_skip_beta", skip_beta),
                    ("d_bias", bias), ("d_resid", resid)):
        if v is not None:
            t = dev(v)
            keep.append(t)
            setattr(a, name, _p(t))
    if skip_st is not None:
        t = dev(skip_st[0], torch.float64)
        keep.append(t)
        a.d_skip_stats, a.skip_slots, a.skip_m_tile, a.skip_n_tiles, a.skip_cnorm = _p(t), *skip_st[1:]
    if resid is not None:
        a.resid_ld = N
    dst = torch.full((M, N), float("nan"), device="cuda")
    a.d_dst, a.dst_ld = _p(dst), N
    cap = B * max(((HW + 14) // 16 + 1) * (N // 16), HW + 1) * 2
    st = torch.empty(cap, dtype=torch.float64, device="cuda")
    a.d_stats, a.stats_cap = _p(st), cap
    rs = None
    if row_stats:
        rs = torch.empty(M * (N // 64) * 2, dtype=torch.float64, device="cuda")
        a.d_row_stats, a.row_stats_cap = _p(rs), rs.numel()
    torch.cuda.synchronize()
    rc = lib.spdm_op_gemm(ctypes.byref(a))
    if not check:
        return rc, lib.spdm_last_error()
    L.check(rc, "spdm_op_gemm")
    out = list(a.out)
    r = dict(kernel=out[0], variant=out[1], m_tile=out[2], n_tile=out[3], ksplit=out[4], two=out[5], fused=out[6],
             slots=out[7], st_m=out[8], st_n=out[9])
    r["out"] = dst.cpu().reshape(B, HW, N) if taps != 1 else dst.cpu()
    if epi == EPI_STATS:
        r["stats"] = st[: B * r["slots"] * 2].cpu().reshape(B, r["slots"], 2)
    if row_stats:
        r["row_stats"] = rs[: M * (N // r["n_tile"]) * 2].cpu().reshape(M, N // r["n_tile"], 2)
    return r


def subset(B, HW, m_tile, seed=0):
    """Samples compared against the CPU reference (all of them when there are few): the first and last, the samples on
    both sides of every tile boundary that crosses a sample -- a seeded 38 of them when there are more than 40, to bound the
    CPU reference's time --, every sample of the ragged last tile, and 8 seeded random ones."""
    if B <= 24:
        return list(range(B))
    M = B * HW
    s = {0, B - 1}
    for k in range(1, (M + m_tile - 1) // m_tile):
        r = k * m_tile
        if r % HW:                                   # the boundary crosses a sample
            s.update({(r - 1) // HW, r // HW})
    if len(s) > 40:
        g = np.random.default_rng(seed)
        s = {0, B - 1} | set(g.choice(sorted(s), 38, replace=False).tolist())
    last = ((M - 1) // m_tile) * m_tile
    s.update(range(last // HW, B))                   # the ragged last tile
    g = np.random.default_rng(seed + 1)
    s.update(g.choice(B, 8, replace=False).tolist())
    return sorted(s)


# ---- data -------------------------------------------------------------------------------------------------------------
def gen(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


def activations(B, rows, C, seed, flavor, cnorm=None):
    """flavor 'edges': per-sample offsets much larger than the spread on half the samples (mean 50, std 0.5 -- the
    E[x^2] - E[x]^2 cancellation of the fp64 partials), one all-zero sample (variance 0: only eps is left);
    'big': |x| up to 3000 (DESIGN.md 4.1's range is < 4094); 'unit': U(-1, 1)."""
    if B * rows * C > 1 << 26:              # (the largest layer shapes: generated in fp32, 0.5 GB instead of 1 GB)
        g = torch.Generator().manual_seed(seed)
        x = torch.rand((B, rows, C), generator=g) * 2 - 1
        if flavor == "edges":
            off = torch.randn(B, 1, 1, generator=g) * 5
            off[::2] = 50.0
            x = off + 0.5 * torch.randn(B, rows, C, generator=g)
            x[B // 2] = 0.0
        return x
    x = gen((B, rows, C), seed)
    if flavor == "edges":
        g = torch.Generator().manual_seed(seed + 7)
        off = torch.randn(B, 1, 1, generator=g, dtype=torch.float64) * 5
        off[::2] = 50.0
        x = off + 0.5 * torch.randn(B, rows, C, generator=g, dtype=torch.float64)
        if B > 1:
            x[B // 2] = 0.0
    elif flavor == "big":
        x = x * 3000.0
    if cnorm is not None and cnorm < C:
        x[..., cnorm:] = 0.0
    return x.float()


def gains(C, seed, flavor, cnorm=None):
    """(gamma, beta); 'edges': negative, exactly zero and positive gains mixed."""
    g = gen((C,), seed, -1.5, 1.5) if flavor == "edges" else gen((C,), seed, 0.5, 1.5)
    if flavor == "edges":
        g[::5] = 0.0
    b = gen((C,), seed + 1, -0.5, 0.5)
    if cnorm is not None and cnorm < C:
        g[cnorm:] = 0.0
        b[cnorm:] = 0.0
    return g.float(), b.float()


def weights(N, K, taps, seed, flavor="unit", kreal=None, nreal=None):
    shape = (N, K) if taps == 1 else (N, K, 3, 3)
    w = gen(shape, seed) * (3.0 / (K * (1 if taps == 1 else 9))) ** 0.5
    if flavor == "big":
        w = gen(shape, seed) * 400.0
    if kreal is not None:
        w[:, kreal:] = 0.0
    if nreal is not None:
        w[nreal:] = 0.0
    return w.float()


# ---- comparison -------------------------------------------------------------------------------------------------------
def compare(r, want, scale, fl, split, idx, tag):
    got = r["out"][idx].double() if r["out"].dim() == 3 else r["out"].double()
    tau = TAU_SPLIT if split else TAU_EXACT
    bound = tau * scale
    if split:
        bound = bound + FLOOR_X * fl[0] + FLOOR_W * fl[1]
    bound = bound + 1e-30
    err = (got - want).abs()
    assert torch.isfinite(got).all(), tag
    ratio = float((err / bound).max())
    print(f"RATIO {tag} {ratio:.4f} (tau {tau:g}, max err {float(err.max()):.3e})")
    assert ratio <= 1.0, (tag, ratio, float(err.max()))
    return ratio


def check_stats(r, B, HW, N, tag, cnorm=None):
    """Per-sample GroupNorm totals from the returned slots against the fp64 totals of the launch's own output."""
    tot = stats_totals(r["stats"], HW, r["st_m"], r["st_n"], B)
    n = HW * (cnorm or N)
    s1, s2 = torch.empty(B, dtype=torch.float64), torch.empty(B, dtype=torch.float64)
    for b0 in range(0, B, 256):
        o = r["out"][b0:b0 + 256].double().reshape(-1, HW * N)
        s1[b0:b0 + 256], s2[b0:b0 + 256] = o.sum(1), (o * o).sum(1)
    mean, msq = s1 / n, s2 / n
    var = msq - mean * mean
    m1, v1 = tot[:, 0] / n, tot[:, 1] / n - (tot[:, 0] / n) ** 2
    assert torch.isfinite(tot).all(), tag
    sig = var.clamp_min(1e-30).sqrt()
    assert float(((m1 - mean).abs() / sig).max()) <= 1e-6, (tag, "mean")
    assert float(((v1 - var).abs() / var.clamp_min(1e-30)).max()) <= 1e-5, (tag, "variance")


def run_case(B, H, W, K, N, taps=9, split=1, pro=PRO_NONE, epi=EPI_STATS, flavor="unit", seed=0, up_C=0, two=False,
             src_gn=True, skip_gn=True, cnorm=None, env=None, expect=None, wflavor=None, src_scale=1.0, w_scale=1.0):
    """Generate a case, run it, compare.  Returns the worst ratio."""
    HW = H * W
    src_rows = 4 * HW if pro == PRO_POOL else HW // 4 if pro == PRO_UPCAT else HW
    src_C = up_C if (pro == PRO_UPCAT or two) else K
    src = activations(B, src_rows, src_C, seed, flavor, cnorm) * src_scale
    if taps == 1:
        src = src.reshape(B, src_C)
    kw = dict(src=src)
    gn = None
    call = {}
    pending = pro in (PRO_GN, PRO_GN_GELU) or (pro in (PRO_POOL, PRO_UPCAT) and src_gn)
    if pending:
        g, b = gains(src_C, seed + 11, flavor, cnorm)
        mt = 64 if src_rows >= 64 else 16
        st, slots = partials(src, mt, 32 if src_C % 32 == 0 else src_C, src_rows)
        call.update(src_st=(st, slots, mt, src_C // 32 if src_C % 32 == 0 else 1, cnorm or src_C), gamma=g, beta=b)
        gn = (g, b, cnorm)
    skip = sgn = None
    if pro == PRO_UPCAT or two:
        skip = activations(B, HW, K - up_C, seed + 21, flavor)
        call.update(skip=skip, up_C=up_C)
        if skip_gn:
            sg, sb = gains(K - up_C, seed + 23, flavor)
            st, slots = partials(skip, 64 if HW >= 64 else 16, 32, HW)
            call.update(skip_st=(st, slots, 64 if HW >= 64 else 16, (K - up_C) // 32, K - up_C), skip_gamma=sg, skip_beta=sb)
            sgn = (sg, sb, None)
    w = weights(N, K, taps, seed + 31, wflavor or ("big" if flavor == "big" else "unit"),
                kreal=cnorm, nreal=None) * w_scale
    bias = gen((N,), seed + 41).float() if epi not in (EPI_STATS, EPI_PLAIN) else None
    resid = gen((B * HW, N), seed + 43).float() if epi == EPI_BIAS_RESID else None
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        r = op_gemm(B, H, W, K, N, taps, split, pro, epi, src, w, bias=bias, resid=resid, **call)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    tag = f"B{B} {H}x{W} K{K} N{N} t{taps} s{split} pro{pro} epi{epi} {flavor} {env or ''} route={[r[k] for k in ('kernel', 'variant', 'm_tile', 'n_tile', 'ksplit')]}"
    for k, v in (expect or {}).items():
        assert r[k] == v, (tag, k, r[k], v)
    idx = subset(B, HW, r["m_tile"]) if taps != 1 else list(range(B))
    sel = lambda t: None if t is None else t[idx]
    xkw = dict(taps=taps, gn=gn, skip=sel(skip), skip_gn=sgn, up_C=up_C)
    if taps == 1:
        want, scale = ref_launch(pro, epi, src, w, H, W, taps=1, gn=gn, bias=bias, resid=resid)
        fl = floor_terms(pro, src, w, H, W, taps=1, gn=gn)
    else:
        rs = None if resid is None else resid.reshape(B, HW, N)[idx]
        want, scale = ref_launch(pro, epi, src[idx], w, H, W, bias=bias, resid=rs, **xkw)
        fl = floor_terms(pro, src[idx], w, H, W, **xkw)
    ratio = compare(r, want, scale, fl, split, idx, tag)
    if epi == EPI_STATS:
        check_stats(r, B, HW, N, tag)
    return r, ratio


# ---- the route matrix ---------------------------------------------------------------------------------------------------
# (B, H, W, K, N, kwargs, expected route)
WIDE_CASES = [
    ((2048, 16, 4, 128, 128), dict(pro=PRO_GN), dict(kernel=WIDE, variant=WP4, m_tile=256)),
    ((600, 16, 4, 128, 128), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=WP4, m_tile=128)),
    ((600, 32, 8, 128, 128), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=WP8, m_tile=256)),
    ((701, 24, 8, 128, 128), dict(pro=PRO_GN), dict(kernel=WIDE, variant=WP8, m_tile=256)),          # HW = 192, ragged
    ((700, 12, 4, 128, 128), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, m_tile=128)),                   # HW = 48
    ((4096, 8, 2, 256, 256), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=W2, m_tile=256)),
    ((4093, 4, 1, 512, 256), dict(taps=3, pro=PRO_GN), dict(kernel=WIDE, m_tile=128)),                # 3-tap, W = 1, ragged
    ((1024, 16, 4, 256, 64), dict(pro=PRO_GN), dict(kernel=WIDE, variant=PIPE, m_tile=256, n_tile=64)),
    ((777, 16, 4, 256, 64), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=PIPE, m_tile=256, n_tile=64)),
    ((600, 16, 4, 256, 128), dict(up_C=128, two=True), dict(kernel=WIDE, variant=WP4, two=1)),         # two-source, skip GN
    ((2048, 8, 2, 512, 256), dict(up_C=256, two=True), dict(kernel=WIDE, variant=W2, two=1)),
    ((2048, 16, 4, 128, 128), dict(pro=PRO_NONE), dict(kernel=WIDE, variant=WP4)),
]
REG_CASES = [
    ((1024, 8, 8, 64, 64), dict(pro=PRO_GN), dict(kernel=REG)),              # 1 wave tile per sample
    ((512, 16, 8, 64, 64), dict(pro=PRO_GN_GELU), dict(kernel=REG)),         # 2
    ((343, 24, 8, 64, 64), dict(pro=PRO_GN_GELU), dict(kernel=REG)),         # 3, ragged last workgroup
    ((512, 32, 8, 64, 64), dict(pro=PRO_NONE), dict(kernel=REG)),            # 4
    ((257, 64, 8, 64, 64), dict(pro=PRO_GN), dict(kernel=REG)),              # 8, ragged
    ((2047, 16, 4, 64, 64), dict(pro=PRO_GN_GELU), dict(kernel=REG)),        # width 4
]
GEMM_CASES = [
    ((8, 32, 8, 128, 128), dict(split=0, pro=PRO_GN), dict(kernel=GEMM)),
    ((8, 32, 8, 128, 64), dict(split=0, pro=PRO_GN_GELU), dict(kernel=GEMM, n_tile=64)),
    ((600, 16, 4, 128, 128), dict(pro=PRO_GN, env={"SPDM_NO_WIDE": "1"}), dict(kernel=GEMM)),
    ((700, 16, 4, 64, 64), dict(pro=PRO_GN_GELU, env={"SPDM_NO_WIDE": "1", "SPDM_NO_REG64": "1"}), dict(kernel=GEMM, n_tile=64)),
    ((1536, 1, 1, 64, 192), dict(taps=1, epi=EPI_BIAS), dict(kernel=GEMM)),
    ((1536, 1, 1, 128, 128), dict(taps=1, epi=EPI_BIAS_GELU), dict(kernel=GEMM)),
    ((1536, 1, 1, 64, 64), dict(taps=1, epi=EPI_BIAS_RESID), dict(kernel=GEMM)),
    ((1000, 1, 1, 256, 256), dict(taps=1, epi=EPI_BIAS_RESID, split=0), dict(kernel=GEMM)),
]
SKINNY_CASES = [((B, H, W, K, N), dict(taps=t, pro=PRO_GN_GELU), dict(kernel=SKINNY))      # (level 0 leaves it above batch 16)
                for (H, W, K, N, t), bs in (((32, 8, 64, 64, 9), (1, 3, 16)), ((16, 4, 128, 128, 9), (1, 3, 64)),
                                            ((8, 2, 256, 256, 9), (1, 3, 64)), ((4, 1, 512, 512, 3), (1, 3, 64))) for B in bs]
SKINNY_CASES += [
    ((2, 16, 4, 64, 128), dict(pro=PRO_POOL), dict(kernel=SKINNY, fused=1)),
    ((8, 8, 2, 128, 256), dict(pro=PRO_POOL, src_gn=False), dict(kernel=SKINNY, fused=1)),
    ((1, 4, 1, 256, 512), dict(taps=3, pro=PRO_POOL), dict(kernel=SKINNY, fused=1)),
    ((2, 16, 4, 384, 128), dict(pro=PRO_UPCAT, up_C=256), dict(kernel=SKINNY, fused=1)),
    ((4, 32, 8, 192, 64), dict(pro=PRO_UPCAT, up_C=128, src_gn=False), dict(kernel=SKINNY, fused=1)),
    ((16, 8, 2, 768, 256), dict(pro=PRO_UPCAT, up_C=512, skip_gn=False), dict(kernel=SKINNY, fused=1)),
]
SPLITK_CASES = [((B, H, W, K, N), dict(taps=t, pro=PRO_GN, env={"SPDM_NO_SKINNY": "1", "SPDM_NO_REG64": "1"}),
                 dict(kernel=GEMM, ksplit=lambda k: k > 1))
                for B in (1, 3, 8, 64) for (H, W, K, N, t) in ((32, 8, 64, 64, 9), (16, 4, 128, 128, 9), (8, 2, 256, 256, 9), (4, 1, 512, 512, 3))]

ALL = ([("wide",) + c for c in WIDE_CASES] + [("reg",) + c for c in REG_CASES] + [("gemm",) + c for c in GEMM_CASES] +
       [("skinny",) + c for c in SKINNY_CASES] + [("splitk",) + c for c in SPLITK_CASES])


@pytest.mark.parametrize("flavor", ["edges", "big"])
@pytest.mark.parametrize("route,shape,kw,expect", ALL, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-{i}" for i, c in enumerate(ALL)])
def test_launch_against_fp64(route, shape, kw, expect, flavor):
    kw = dict(kw)
    if flavor == "big":          # |activation| up to 3000 is a raw (PRO_NONE) input: no GroupNorm pending on any source
        if kw.get("pro", PRO_NONE) in (PRO_GN, PRO_GN_GELU):
            kw["pro"] = PRO_NONE
        kw["src_gn"] = kw["skip_gn"] = False
    exp = {k: v for k, v in expect.items() if not callable(v)}
    r, _ = run_case(*shape, flavor=flavor, expect=exp, **kw)
    for k, v in expect.items():
        if callable(v):
            assert v(r[k]), (shape, k, r[k])


SWEEP = [((2048, 16, 4, 128, 128), {}, dict(kernel=WIDE)), ((2, 8, 2, 256, 256), {}, dict(kernel=SKINNY)),
         ((512, 32, 8, 64, 64), {}, dict(kernel=REG)),
         ((600, 16, 4, 128, 128), dict(env={"SPDM_NO_WIDE": "1"}), dict(kernel=GEMM, ksplit=1)),
         ((3, 16, 4, 128, 128), dict(env={"SPDM_NO_SKINNY": "1", "SPDM_NO_REG64": "1"}), dict(kernel=GEMM, ksplit=4)),
         ((1536, 1, 1, 128, 128), dict(taps=1, epi=EPI_PLAIN), dict(kernel=GEMM))]


@pytest.mark.parametrize("e", list(range(-12, 9, 2)))
@pytest.mark.parametrize("shape,kw,expect", SWEEP, ids=["wide", "skinny", "reg", "gemm3x3", "splitk", "linear"])
def test_scale_sweep(shape, kw, expect, e):
    """PRO_NONE input and weights scaled by 2^e, e = -12 .. 8, on every route: the error stays under the split format's bound
    (relative TAU_SPLIT plus the subnormal-lo floors) at every scale."""
    run_case(*shape, flavor="unit", expect=expect, src_scale=2.0 ** e, w_scale=2.0 ** e, **kw)


def test_chained_double_conv_small_and_large_grid():
    """conv1 (EPI_STATS) -> conv2 (PRO_GN_GELU reading conv1's multi-slot partials) -> GroupNorm affine from conv2's partials,
    against the oracle's DoubleConvolution in float64."""
    from oracle.unet_film_ref import double_conv
    for B, H, W, C, kern in ((2, 16, 4, 128, SKINNY), (1024, 16, 4, 128, WIDE)):
        HW = H * W
        x = activations(B, HW, C, 5, "edges")
        g, b = gains(C, 6, "edges")
        w1, w2 = weights(C, C, 9, 7), weights(C, C, 9, 8)
        r1 = op_gemm(B, H, W, C, C, 9, 1, PRO_NONE, EPI_STATS, x, w1)
        assert r1["kernel"] == kern, r1["kernel"]
        st1 = (r1["stats"], r1["slots"], r1["st_m"], r1["st_n"], C)
        r2 = op_gemm(B, H, W, C, C, 9, 1, PRO_GN_GELU, EPI_STATS, r1["out"], w2, src_st=st1, gamma=g, beta=b)
        tot = stats_totals(r2["stats"], HW, r2["st_m"], r2["st_n"], B)
        n = HW * C
        mean = tot[:, 0] / n
        var = tot[:, 1] / n - mean * mean
        y = (r2["out"].double() - mean[:, None, None]) / (var[:, None, None] + 1e-5).sqrt() * g.double() + b.double()
        idx = subset(B, HW, r2["m_tile"])
        sd = {"p.first.weight": w1.double(), "p.second.weight": w2.double(), "p.norm.weight": g.double(), "p.norm.bias": b.double()}
        xn = x[idx].double().reshape(len(idx), H, W, C).permute(0, 3, 1, 2)
        want = double_conv(sd, "p", xn).permute(0, 2, 3, 1).reshape(len(idx), HW, C)
        err = float((y[idx] - want).abs().max())
        print(f"RATIO chained B{B} max err {err:.3e}")
        assert err <= 1.5e-5, (B, err)          # measured 1.7e-6 (B = 2) and 4.8e-6 (B = 1024)


def test_simple_unet_padded_channels():
    """Channel counts that are not multiples of 64, padded as plan_simple stores them: zero weight lanes, zero gain and
    offset, statistics over the real channel count."""
    B, H, W, Kp, Np, k, n = 64, 16, 4, 64, 64, 48, 40
    HW = H * W
    x = activations(B, HW, Kp, 3, "edges", cnorm=k)
    g, b = gains(Kp, 4, "edges", cnorm=k)
    st, slots = partials(x, 64, 32, HW)
    w = weights(Np, Kp, 9, 5, kreal=k, nreal=n)
    r = op_gemm(B, H, W, Kp, Np, 9, 1, PRO_GN_GELU, EPI_STATS, x, w, src_st=(st, slots, 64, 2, k), gamma=g, beta=b)
    want, scale = ref_launch(PRO_GN_GELU, EPI_STATS, x, w, H, W, gn=(g, b, k))
    fl = floor_terms(PRO_GN_GELU, x, w, H, W, gn=(g, b, k))
    compare(r, want, scale, fl, 1, list(range(B)), "simple-unet padded")
    assert float(r["out"][..., n:].abs().max()) == 0.0
    check_stats(r, B, HW, Np, "simple-unet padded", cnorm=n)


# The convolution shapes of the network's levels 0-3 (H x W, Cin -> Cout, taps) at the published batch sizes, with the route each
# takes: B = 640 / 768 / 896 at H = 32 (the ragged 384-workgroup grids of DESIGN.md 9.5) and B = 4096 at H = 64, D = 6 (config 5).
def _published(B, H):
    L0, L1, L2, L3 = (H, 8), (H // 2, 4), (H // 4, 2), (H // 8, 1)
    mid = B == 640        # level 1, 256 -> 64: 128-row conv_gemm tiles at 640, pipelined 256 x 64 conv_wide tiles above
    big = B == 4096
    return [
        (L0, 64, 64, 9, dict(kernel=REG)),
        (L0, 128, 64, 9, dict(kernel=WIDE, variant=PLAIN, m_tile=256, n_tile=64)),
        (L1, 128, 128, 9, dict(kernel=WIDE, variant=WP4, m_tile=256 if big else 128, n_tile=128)),
        (L1, 256, 64, 9, dict(kernel=GEMM, variant=PLAIN, m_tile=128, n_tile=64) if mid else dict(kernel=WIDE, variant=PIPE, m_tile=256, n_tile=64)),
        (L2, 256, 256, 9, dict(kernel=WIDE, variant=W2, m_tile=256, n_tile=128, ksplit=1 if big else {640: 4, 768: 3, 896: 3}[B])),
        (L2, 512, 128, 9, dict(kernel=WIDE, variant=W2, m_tile=256, n_tile=128, ksplit=1 if big else {640: 7, 768: 6, 896: 5}[B])),
        (L3, 512, 512, 3, dict(kernel=GEMM, variant=PLAIN, m_tile=256, n_tile=128, ksplit=1) if big else dict(kernel=GEMM, variant=PLAIN, m_tile=128, n_tile=64, ksplit=2)),
        (L3, 256, 512, 3, dict(kernel=GEMM, variant=PLAIN, m_tile=256, n_tile=128, ksplit=1) if big else dict(kernel=GEMM, variant=PLAIN, m_tile=128, n_tile=64, ksplit=2)),
    ]


PUBLISHED = [(B, H) + c for B, H in ((640, 32), (768, 32), (896, 32), (4096, 64)) for c in _published(B, H)]


@pytest.mark.parametrize("B,H,hw,K,N,taps,expect", PUBLISHED,
                         ids=[f"B{c[0]}-{c[2][0]}x{c[2][1]}-{c[3]}to{c[4]}" for c in PUBLISHED])
def test_published_layer_shapes(B, H, hw, K, N, taps, expect):
    run_case(B, hw[0], hw[1], K, N, taps=taps, pro=PRO_GN_GELU, flavor="edges", expect=expect)


def test_linear_layernorm_prologue_and_row_stats():
    """The attention blocks' chain: a Linear that writes per-row statistics of its output (row_stats, [row][n_tiles][2]), and
    the Linear whose LayerNorm prologue reads them in the plan's layout (Ctx::row_stats_alloc: slots = the producer's n-tiles,
    m_tile = 1 << 30, one "sample" per row)."""
    rows, C, N = 1000, 128, 128
    x = activations(rows, 1, C, 9, "edges").reshape(rows, C)
    w0, b0 = weights(C, C, 1, 8), gen((C,), 7).float()
    p = op_gemm(rows, 1, 1, C, C, 1, 1, PRO_NONE, EPI_BIAS, x, w0, bias=b0, row_stats=True)
    assert p["kernel"] == GEMM
    y = p["out"]
    want, scale = ref_launch(PRO_NONE, EPI_BIAS, x, w0, 1, 1, taps=1, bias=b0)
    compare(p, want, scale, floor_terms(PRO_NONE, x, w0, 1, 1, taps=1), 1, None, "linear -> row_stats")
    yd = y.double()
    rs = p["row_stats"].sum(1) / C                  # per-row LayerNorm statistics of the stored values, the existing gates
    mean, var = yd.mean(1), yd.var(1, unbiased=False)
    assert float(((rs[:, 0] - mean).abs() / var.sqrt()).max()) <= 1e-6
    assert float(((rs[:, 1] - rs[:, 0] ** 2 - var).abs() / var).max()) <= 1e-5
    n_tiles = p["row_stats"].shape[1]
    g, b = gains(C, 10, "edges")
    w = weights(N, C, 1, 11)
    bias = gen((N,), 12).float()
    r = op_gemm(rows, 1, 1, C, N, 1, 1, PRO_GN, EPI_BIAS, y, w, src_st=(p["row_stats"], n_tiles, 1 << 30, n_tiles, C),
                gamma=g, beta=b, bias=bias)
    assert r["kernel"] == GEMM
    want, scale = ref_launch(PRO_GN, EPI_BIAS, y, w, 1, 1, taps=1, gn=(g, b, None), bias=bias)
    compare(r, want, scale, floor_terms(PRO_GN, y, w, 1, 1, taps=1, gn=(g, b, None)), 1, None, "row_stats -> linear LN")


def test_invalid_combinations_are_refused():
    x = activations(2, 64, 64, 0, "unit")
    w = weights(64, 64, 9, 0)
    rc, msg = op_gemm(2, 8, 8, 64, 96, 9, 1, PRO_NONE, EPI_STATS, x, weights(96, 64, 9, 0), check=False)
    assert rc == -1 and b"N % 64" in msg
    rc, msg = op_gemm(1024, 8, 2, 128, 128, 9, 1, PRO_POOL, EPI_STATS, activations(1024, 64, 128, 0, "unit"),
                      weights(128, 128, 9, 0), check=False)
    assert rc == -1 and b"fused source" in msg
    rc, msg = op_gemm(2, 8, 8, 64, 64, 9, 1, PRO_GN, EPI_STATS, x, w, check=False)
    assert rc == -1


def test_split_range_verdict_at_the_smallest_conv_shape():
    """spdm_op_gemm lays its weights out through the device weight-copy table, so the split format's range verdict is the
    WL_RANGE kernel's (weight_layout.hip): !(|w| < 511), NaN included, refuses the launch; 510 is accepted and the output meets
    this file's bound.  The marked weight sits in the centre column, the one a 3-tap launch reads."""
    B, H, W, K, N, taps = 1, 8, 1, 32, 64, 3
    x = activations(B, H * W, K, 2, "unit")
    w = weights(N, K, taps, 3)
    for bad in (600.0, float("nan")):
        wb = w.clone()
        wb[5, 7, 2, 1] = bad
        rc, msg = op_gemm(B, H, W, K, N, taps, 1, PRO_NONE, EPI_STATS, x, wb, check=False)
        assert rc == -1 and b"op_gemm: weights outside the split format's range" in msg, (bad, rc, msg)
    centre = w[:, :, :, 1]
    centre.view(-1)[centre.abs().argmax()] = 510.0           # (a view: w itself changes)
    assert float(w.abs().max()) == 510.0
    r = op_gemm(B, H, W, K, N, taps, 1, PRO_NONE, EPI_STATS, x, w)
    want, scale = ref_launch(PRO_NONE, EPI_STATS, x, w, H, W, taps=taps)
    compare(r, want, scale, floor_terms(PRO_NONE, x, w, H, W, taps=taps), 1, list(range(B)), "range: |w| max 510")
