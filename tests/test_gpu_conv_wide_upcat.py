"""conv3x3_wide_kernel's upsampling slab loader (csrc/conv_wide.hip, template parameter UP: pro = PRO_UPCAT at large batch)
against the path it replaces, upcat_kernel followed by the two-source launch.

On whole-sample two-source tiles of 256 rows the chunks [0, up_C / 32) are formed inside the loader from the coarser level's
raw tensor: its pending GroupNorm applied once per coarse element, the rows parked in LDS, every staged row the align_corners
blend of four LDS neighbours (csrc/resample.h, the arithmetic upcat_kernel shares).  The upsampled value passes through the
two-source loader unchanged, so both paths must give the SAME BITS -- output and GroupNorm partials -- and the fused launch
must meet tests/test_gpu_gemm_fp64.py's bound against the float64 reference (tests/gemm_ref.py, PRO_UPCAT).  Everything that
is not such a tile keeps the materialised path: the fused-source query says no.  SPDM_TUNE22=0 (read once per process)
restores the materialised path everywhere.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_gemm_fp64 as G
from gemm_ref import EPI_STATS, PRO_NONE, PRO_UPCAT, floor_terms, partials, ref_launch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "SPDM_TUNE22"
WIDE, W2, WP4, WP8 = G.WIDE, G.W2, G.WP4, G.WP8


def upsample(coarse, Hin, Win, gn_call):
    """upcat_kernel alone (no skip half) through the stream-ops hook: (B, 4 Hin Win, C) float32, the bits the plan's
    materialised path hands to the two-source launch."""
    L, lib = G._lib()
    B, _, C = coarse.shape
    a = L.SpdmOpStreamArgs()
    a.op = L.OP_STREAM_OPS.index("upcat")
    for i, v in enumerate((B, Hin, Win, C, 0)):
        a.dim[i] = v
    src = coarse.float().contiguous().cuda()
    out = torch.full((B * 4 * Hin * Win * C,), float("nan"), device="cuda")
    a.d_buf[0], a.cap[0] = src.data_ptr(), src.numel()
    a.d_buf[2], a.cap[2] = out.data_ptr(), out.numel()
    keep = []
    if gn_call:
        st, slots, mt, nt, cnorm = gn_call["src_st"]
        st = st.to(torch.float64).contiguous().cuda()
        ga, be = gn_call["gamma"].float().cuda(), gn_call["beta"].float().cuda()
        keep += [st, ga, be]
        a.gn[0].d_stats, a.gn[0].stats_cap = st.data_ptr(), st.numel()
        a.gn[0].slots, a.gn[0].m_tile, a.gn[0].n_tiles, a.gn[0].cnorm = slots, mt, nt, cnorm
        a.gn[0].d_gamma, a.gn[0].d_beta, a.gn[0].affine_cap = ga.data_ptr(), be.data_ptr(), ga.numel()
    torch.cuda.synchronize()
    L.check(lib.spdm_op_stream(ctypes.byref(a)), "spdm_op_stream(upcat)")
    return out.cpu().reshape(B, 4 * Hin * Win, C)


def run_pair(B, H, W, K, N, up_C, coarse_gn, variant, seed=0, coarse=None, st_tile=None):
    """(a) PRO_UPCAT on the coarse source, (b) upcat then the two-source launch: same bits; (a) under the fp64 bound."""
    HW, Hin, Win = H * W, H // 2, W // 2
    rows = HW // 4
    if coarse is None:
        coarse = G.activations(B, rows, up_C, seed, "edges")
    skip = G.activations(B, HW, K - up_C, seed + 21, "edges")
    sg, sb = G.gains(K - up_C, seed + 23, "edges")
    mt = 64 if HW >= 64 else 16
    st, slots = partials(skip, mt, 32, HW)
    skip_call = dict(skip=skip, up_C=up_C, skip_st=(st, slots, mt, (K - up_C) // 32, K - up_C), skip_gamma=sg, skip_beta=sb)
    gn, gn_call = None, {}
    if coarse_gn:
        g, b = G.gains(up_C, seed + 11, "edges")
        cmt, cnt = st_tile or (16 if rows >= 16 else rows, 32)
        cst, cslots = partials(coarse, cmt, cnt, rows)
        gn_call = dict(src_st=(cst, cslots, cmt, up_C // cnt, up_C), gamma=g, beta=b)
        gn = (g, b, None)
    w = G.weights(N, K, 9, seed + 31)
    fused = G.op_gemm(B, H, W, K, N, 9, 1, PRO_UPCAT, EPI_STATS, coarse, w, **skip_call, **gn_call)
    up = upsample(coarse, Hin, Win, gn_call)
    two = G.op_gemm(B, H, W, K, N, 9, 1, PRO_NONE, EPI_STATS, up, w, **skip_call)
    tag = f"B{B} {H}x{W} K{K} N{N} up_C{up_C} gn{int(coarse_gn)} route={[fused[k] for k in ('kernel', 'variant', 'm_tile', 'n_tile', 'ksplit', 'fused')]}"
    for r, want in ((fused, dict(kernel=WIDE, variant=variant, m_tile=256, n_tile=128, ksplit=1, fused=1, two=0)),
                    (two, dict(kernel=WIDE, variant=variant, m_tile=256, n_tile=128, ksplit=1, fused=0, two=1))):
        for k, v in want.items():
            assert r[k] == v, (tag, k, r[k], v)
    assert torch.equal(fused["out"].view(torch.int32), two["out"].view(torch.int32)), (tag, "dst bits differ")
    assert torch.equal(fused["stats"].view(torch.int64), two["stats"].view(torch.int64)), (tag, "statistics partials differ")
    idx = G.subset(B, HW, 256)
    xkw = dict(taps=9, gn=gn, skip=skip[idx], skip_gn=(sg, sb, None), up_C=up_C)
    want, scale = ref_launch(PRO_UPCAT, EPI_STATS, coarse[idx], w, H, W, **xkw)
    fl = floor_terms(PRO_UPCAT, coarse[idx], w, H, W, **xkw)
    G.compare(fused, want, scale, fl, 1, idx, tag)
    G.check_stats(fused, B, HW, N, tag)


# the smallest batches whose launch is conv_wide's 256-row whole-sample tiling in each layout: (B, H, W, K, N), up_C, variant
LAYOUTS = [((320, 32, 8, 128, 128), 64, WP8), ((520, 16, 4, 256, 256), 128, WP4), ((1040, 8, 2, 512, 512), 256, W2)]


@pytest.mark.parametrize("coarse_gn", [True, False], ids=["coarse_gn", "coarse_final"])
@pytest.mark.parametrize("shape,up_C,variant", LAYOUTS, ids=["width8", "width4", "width2"])
def test_fused_upsample_matches_upcat_then_two_source_bitwise(shape, up_C, variant, coarse_gn):
    run_pair(*shape, up_C, coarse_gn, variant)


def test_many_partial_slots_of_the_coarse_tensor():
    """16 slots per sample of the coarse tensor: the statistics go through the wave-wide sum, as in upcat_kernel."""
    run_pair(320, 32, 8, 128, 128, 64, True, WP8, seed=3, st_tile=(16, 16))


def test_edge_clamp_and_sample_addressing():
    """Width 8, one sample per tile, a distinct seed per sample and outliers in the last coarse row and column: the clamp of
    the second source index at the map's edge, and the sample a tile takes its coarse rows from."""
    B, H, W, up_C = 320, 32, 8, 64
    Hin, Win = H // 2, W // 2
    coarse = torch.stack([G.gen((Hin * Win, up_C), 1000 + b) * (1.0 + 0.01 * b) for b in range(B)]).float()
    c = coarse.reshape(B, Hin, Win, up_C)
    c[:, Hin - 1, :, :] = c[:, Hin - 1, :, :] * 7.0 + 3.0           # last coarse row
    c[:, :, Win - 1, :] = c[:, :, Win - 1, :] * -5.0 - 2.0          # last coarse column
    run_pair(B, H, W, 128, 128, up_C, True, WP8, seed=5, coarse=c.reshape(B, Hin * Win, up_C).contiguous())


@pytest.mark.parametrize("shape", [(701, 24, 8, 128, 128), (601, 16, 4, 128, 128)], ids=["HW192", "ragged"])
def test_other_tilings_keep_the_materialised_path(shape):
    """HW = 192 does not divide the tile; M % 256 != 0 leaves a ragged last tile: the fused-source query says no (the plan then
    materialises the upsample), and the two-source launch the plan falls back to is still offered."""
    B, H, W, K, N = shape
    up_C, HW = K // 2, H * W
    coarse = G.activations(B, HW // 4, up_C, 0, "unit")
    skip = G.activations(B, HW, K - up_C, 1, "unit")
    w = G.weights(N, K, 9, 2)
    rc, msg = G.op_gemm(B, H, W, K, N, 9, 1, PRO_UPCAT, EPI_STATS, coarse, w, skip=skip, up_C=up_C, check=False)
    assert rc == -1 and b"does not take a fused source" in msg, (rc, msg)
    up = upsample(coarse, H // 2, W // 2, {})
    r = G.op_gemm(B, H, W, K, N, 9, 1, PRO_NONE, EPI_STATS, up, w, skip=skip, up_C=up_C)
    assert r["kernel"] == WIDE and r["two"] == 1 and r["fused"] == 0, r


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from state_policy_diffusionmodel_amd.engine import SpdmEngine
from state_policy_diffusionmodel_amd.schedulers import DDPMScheduler
from state_policy_diffusionmodel_amd.weights import random_state_dict
B, H, D, obs_h, obs_dim, N = 320, 32, 3, 2, 7, 2
sd = random_state_dict(obs_h * obs_dim, seed=5)
g = torch.Generator().manual_seed(1)
cond = torch.randn(B, 1, obs_h, obs_dim, generator=g).cuda()
x_T = torch.rand(B, 1, H, D, generator=g).cuda()
noise = torch.randn(N, B, 1, H, D, generator=g).cuda()
eng = SpdmEngine(H, D, obs_h * obs_dim, max_batch=B, num_train_timesteps=N)
eng.load_state_dict(sd)
sched = DDPMScheduler(num_train_timesteps=N)
sched.set_timesteps(N)
eng.set_scheduler(sched)
_, hist = eng.sample(cond, x_T, noise=noise, history=True)
from state_policy_diffusionmodel_amd import _lib
torch.save({"hist": hist.cpu(), "fused": int(_lib.load().spdm_debug_fused_upsample_launches())}, sys.argv[2])
eng.close()
"""


def test_model_iterates_identical_with_and_without_the_knob(tmp_path):
    """B = 320, horizon 32, state_dim 3, two DDPM steps in two fresh processes (the knob is read once per process): every
    iterate bit for bit the same with the upsample in the loader (default) and materialised (SPDM_TUNE22=0)."""
    hists = []
    for name, knob in (("on", None), ("off", "0")):
        env = {k: v for k, v in os.environ.items() if k != KNOB}
        if knob is not None:
            env[KNOB] = knob
        out = tmp_path / f"hist_{name}.pt"
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        got = torch.load(out)
        # level 0 of this batch is a whole-sample 256-row tiling: the plan must have skipped (on) / kept (off) its upcat launch
        assert (got["fused"] > 0) == (knob is None), (name, got["fused"])
        hists.append(got["hist"])
    assert hists[0].shape[0] == 3 and torch.isfinite(hists[0]).all()
    assert torch.equal(hists[0].view(torch.int32), hists[1].view(torch.int32))
