"""conv3x3_wide_kernel's whole-sample staging (csrc/conv_wide.hip, template parameter WH) against the halo'd staging it
replaces on tiles that hold whole samples.

Where M_T % HW == 0 and M % M_T == 0 the rows above and below a tile belong to other samples, every tap that would reach
them is masked, and the slab is staged without its halo rows, clamps and validity select.  The arithmetic per staged element
is unchanged, so the launch must give the SAME BITS as with SPDM_NO_WHOLE_TILES=1 (the old staging) -- output and GroupNorm
partials -- and both must meet tests/test_gpu_gemm_fp64.py's bound against the float64 reference (tests/gemm_ref.py).
spdm_debug_whole_tiles() says which staging ran: 0 halo'd, 1 whole-sample tiles, 2 one sample per tile with a prologue.
"""
import ctypes
import os

import pytest
import torch

import test_gpu_gemm_fp64 as G
from gemm_ref import EPI_STATS, PRO_GN, PRO_GN_GELU, PRO_NONE, floor_terms, partials, ref_launch

pytestmark = pytest.mark.gpu

SWITCH = "SPDM_NO_WHOLE_TILES"


def _launch(env, *args, **kw):
    old = os.environ.get(SWITCH)
    if env:
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)
    try:
        r = G.op_gemm(*args, **kw)
        r["whole"] = int(G._lib()[1].spdm_debug_whole_tiles())
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old
    return r


def run_pair(B, H, W, K, N, taps=9, pro=PRO_NONE, up_C=0, expect=None, whole=0, seed=0):
    """One launch on 'edges' data with the default switches and one with the old staging: same bits, fp64 bound, staging."""
    HW = H * W
    two = up_C > 0
    src_C = up_C if two else K
    src = G.activations(B, HW, src_C, seed, "edges")
    call, gn, skip, sgn = {}, None, None, None
    if pro in (PRO_GN, PRO_GN_GELU):
        g, b = G.gains(src_C, seed + 11, "edges")
        mt = 64 if HW >= 64 else 16
        st, slots = partials(src, mt, 32, HW)
        call.update(src_st=(st, slots, mt, src_C // 32, src_C), gamma=g, beta=b)
        gn = (g, b, None)
    if two:                                             # finished upsampled half + skip half with its pending GroupNorm
        skip = G.activations(B, HW, K - up_C, seed + 21, "edges")
        sg, sb = G.gains(K - up_C, seed + 23, "edges")
        mt = 64 if HW >= 64 else 16
        st, slots = partials(skip, mt, 32, HW)
        call.update(skip=skip, up_C=up_C, skip_st=(st, slots, mt, (K - up_C) // 32, K - up_C), skip_gamma=sg, skip_beta=sb)
        sgn = (sg, sb, None)
    w = G.weights(N, K, taps, seed + 31)
    new = _launch(False, B, H, W, K, N, taps, 1, pro, EPI_STATS, src, w, **call)
    ref = _launch(True, B, H, W, K, N, taps, 1, pro, EPI_STATS, src, w, **call)
    tag = f"B{B} {H}x{W} K{K} N{N} t{taps} pro{pro} two{int(two)} route={[new[k] for k in ('kernel', 'variant', 'm_tile', 'n_tile', 'ksplit')]} whole={new['whole']}"
    for k, v in (expect or {}).items():
        assert new[k] == v and ref[k] == v, (tag, k, new[k], ref[k], v)
    assert new["whole"] == whole, (tag, "staging", new["whole"], whole)
    assert ref["whole"] == 0, (tag, "the switch must force the halo'd staging", ref["whole"])
    assert torch.equal(new["out"].view(torch.int32), ref["out"].view(torch.int32)), (tag, "dst bits differ")
    assert torch.equal(new["stats"].view(torch.int64), ref["stats"].view(torch.int64)), (tag, "statistics partials differ")
    idx = G.subset(B, HW, new["m_tile"])
    xkw = dict(taps=taps, gn=gn, skip=None if skip is None else skip[idx], skip_gn=sgn, up_C=up_C)
    want, scale = ref_launch(pro, EPI_STATS, src[idx], w, H, W, **xkw)
    fl = floor_terms(pro, src[idx], w, H, W, **xkw)
    G.compare(new, want, scale, fl, 1, idx, tag)
    G.check_stats(new, B, HW, N, tag)


WIDE, W2, WP4, WP8, PIPE, PLAIN = G.WIDE, G.W2, G.WP4, G.WP8, G.PIPE, G.PLAIN
# (B, H, W, K, N), kwargs, expected route, expected staging
WHOLE_CASES = [
    ((320, 32, 8, 128, 128), dict(pro=PRO_GN), dict(kernel=WIDE, variant=WP8, m_tile=256), 2),           # one sample per tile
    ((320, 32, 8, 128, 128), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=WP8, m_tile=256), 2),
    ((320, 32, 8, 128, 128), dict(up_C=64), dict(kernel=WIDE, variant=WP8, m_tile=256, two=1), 2),       # two-source, skip GroupNorm
    ((2048, 16, 4, 128, 128), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=WP4, m_tile=256), 1),     # 4 samples per tile
    ((600, 16, 4, 128, 128), dict(pro=PRO_GN), dict(kernel=WIDE, variant=WP4, m_tile=128), 1),           # 2
    ((1024, 16, 4, 256, 64), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=PIPE, m_tile=256, n_tile=64), 1),
    ((320, 32, 8, 128, 64), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=PLAIN, m_tile=256, n_tile=64), 2),
    ((320, 32, 8, 128, 64), dict(pro=PRO_NONE), dict(kernel=WIDE, variant=PLAIN, m_tile=256, n_tile=64), 1),   # no prologue: 1
    ((4096, 8, 2, 256, 256), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=W2, m_tile=256), 1),       # 16 samples per tile
    ((4096, 4, 1, 256, 256), dict(taps=3, pro=PRO_GN), dict(kernel=WIDE, m_tile=128), 1),                # 32 samples per tile
]
FALLBACK_CASES = [
    ((701, 24, 8, 128, 128), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=WP8, m_tile=256), 0),      # HW = 192 does not divide the tile
    ((601, 16, 4, 128, 128), dict(pro=PRO_GN_GELU), dict(kernel=WIDE, variant=WP4), 0),                  # M % 256 != 0: ragged last tile
    ((300, 64, 8, 128, 128), dict(pro=PRO_GN), dict(kernel=WIDE, m_tile=256), 0),                        # HW = 512 exceeds the tile
]


def _id(c):
    (B, H, W, K, N), kw = c[0], c[1]
    return f"B{B}_{H}x{W}_{K}to{N}_" + "_".join(f"{k}{v}" for k, v in kw.items())


@pytest.mark.parametrize("case", WHOLE_CASES, ids=_id)
def test_whole_sample_staging_matches_halo_staging_bitwise(case):
    shape, kw, route, whole = case
    run_pair(*shape, expect=route, whole=whole, **kw)


@pytest.mark.parametrize("case", FALLBACK_CASES, ids=_id)
def test_other_tilings_keep_the_halo_staging(case):
    shape, kw, route, whole = case
    run_pair(*shape, expect=route, whole=whole, **kw)


def test_model_iterates_identical_with_and_without_the_switch():
    """B = 320, horizon 32, state_dim 3, two DDPM steps: every iterate bit for bit the same."""
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    from state_policy_diffusionmodel_amd.schedulers import DDPMScheduler
    from state_policy_diffusionmodel_amd.weights import random_state_dict

    B, H, D, obs_h, obs_dim, N = 320, 32, 3, 2, 7, 2
    sd = random_state_dict(obs_h * obs_dim, seed=5)
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(B, 1, obs_h, obs_dim, generator=g).cuda()
    x_T = torch.rand(B, 1, H, D, generator=g).cuda()
    noise = torch.randn(N, B, 1, H, D, generator=g).cuda()
    hists = []
    for off in (False, True):
        old = os.environ.get(SWITCH)
        if off:
            os.environ[SWITCH] = "1"
        else:
            os.environ.pop(SWITCH, None)
        try:
            eng = SpdmEngine(H, D, obs_h * obs_dim, max_batch=B, num_train_timesteps=N)
        finally:
            if old is None:
                os.environ.pop(SWITCH, None)
            else:
                os.environ[SWITCH] = old
        eng.load_state_dict(sd)
        sched = DDPMScheduler(num_train_timesteps=N)
        sched.set_timesteps(N)
        eng.set_scheduler(sched)
        _, hist = eng.sample(cond, x_T, noise=noise, history=True)
        hists.append(hist.cpu())
        eng.close()
    assert hists[0].shape[0] == N + 1 and torch.isfinite(hists[0]).all()
    assert torch.equal(hists[0].view(torch.int32), hists[1].view(torch.int32))
