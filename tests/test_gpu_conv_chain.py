"""The level-3 convolution chains as one kernel per 64-row block (csrc/conv_chain.hip).

1. One fused launch (spdm_op_chain) against float64 (tests/level3_chain_ref.py).  The yardstick is the per-layer path: the same
   layers run one by one through spdm_op_gemm on the same data.  Both maximum errors are taken against float64, relative to the
   output's absolute maximum, and the fused error must be <= 2 x the per-layer error: the two paths evaluate the same split
   products and differ in summation order and in where the statistics are summed, which the factor 2 covers.  The measured
   pairs are recorded in tests/golden/conv_chain_tau.json.  The statistics slots against float64 sums of the launch's own
   output, at tests/test_gpu_gemm_fp64.py's tolerance for statistics.
2. No tap crosses a sample and no row past M counts: with one sample's input 100 x larger, every OTHER sample's output and
   statistics keep their bits.
3. The same call twice gives the same bits.
4. The whole model with the route forced (SPDM_TUNE25=7, read once per process: fresh processes) against the oracle at
   tests/test_gpu_parity.py's tolerance; the launch counter rises by 2 per evaluation, and by 0 -- with eps equal to the
   SPDM_TUNE25=0 process's bit for bit -- for a geometry the shape rule refuses and on a debug-tap handle.  (The refused
   geometry is horizon 16, whose coarsest map has 2 rows per sample: spdm_create takes no state_dim above 8, so a handle whose
   coarsest map is 2 wide cannot be made.)
5. A 4-step sampling loop with the route forced: the same iterates replayed as a hipGraph and with plain launches.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import level3_chain_ref as R
import test_gpu_gemm_fp64 as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "SPDM_TUNE25"
TOL = 1e-4                                   # tests/test_gpu_parity.py
DOWN3 = (256, 256, 256, 256, 256)
BOT = (256, 512, 512, 512, 512, 256, 256)
NARROW = (64, 128, 64)                       # waves without a full column strip
LISTS = {"down3": DOWN3, "bot": BOT, "narrow": NARROW}
SHAPES = [(4, 16), (4, 20), (4, 33), (8, 8), (8, 9)]          # (HW, B): one block, ragged (four live samples), three blocks


def make_case(chan, HW, B, seed=0):
    """inputs N(0, 1), weights at the scale of random_state_dict (U(+-1 / sqrt(fan_in)), fan_in = 9 Cin), gains of mixed sign"""
    g = np.random.default_rng(seed + 1000 * HW + B)
    n = len(chan) - 1
    x = g.standard_normal((B, HW, chan[0])).astype(np.float32)
    w = [g.uniform(-1, 1, (3, chan[i + 1], chan[i])).astype(np.float32) / np.float32(np.sqrt(9 * chan[i])) for i in range(n)]
    gamma = [None] + [g.uniform(-1.5, 1.5, chan[i]).astype(np.float32) for i in range(1, n)]
    beta = [None] + [g.uniform(-0.5, 0.5, chan[i]).astype(np.float32) for i in range(1, n)]
    gelus = [i % 2 for i in range(n)]        # the plan's pattern: GELU in front of every DoubleConvolution's second layer
    return dict(chan=chan, HW=HW, B=B, x=x, w=w, gamma=gamma, beta=beta, gelus=gelus)


def op_chain(c, x=None):
    L, lib = G._lib()
    n, B, HW = len(c["chan"]) - 1, c["B"], c["HW"]
    a = L.SpdmOpChainArgs()
    a.B, a.HW, a.n_layers = B, HW, n
    for i, ch in enumerate(c["chan"]):
        a.chan[i] = ch
    keep = []
    src = torch.from_numpy(np.ascontiguousarray(c["x"] if x is None else x)).reshape(B * HW, c["chan"][0]).cuda()
    a.d_src, a.src_ld = G._p(src), c["chan"][0]
    for i in range(n):
        a.gelu[i] = c["gelus"][i]
        w = np.ascontiguousarray(c["w"][i], np.float32)
        keep.append(w)
        a.h_weight[i] = w.ctypes.data_as(ctypes.c_void_p)
        if i:
            gm, bt = torch.from_numpy(c["gamma"][i]).cuda(), torch.from_numpy(c["beta"][i]).cuda()
            keep += [gm, bt]
            a.d_gamma[i], a.d_beta[i] = G._p(gm), G._p(bt)
    N = c["chan"][-1]
    extra = 64                                # rows past M: must stay NaN
    dst = torch.full((B * HW + extra, N), float("nan"), device="cuda")
    st = torch.empty(B * 2 * 2, dtype=torch.float64, device="cuda")
    a.d_dst, a.dst_ld, a.d_stats, a.stats_cap = G._p(dst), N, G._p(st), st.numel()
    torch.cuda.synchronize()
    L.check(lib.spdm_op_chain(ctypes.byref(a)), "spdm_op_chain")
    blocks, slots, mt, nt = list(a.out)
    assert (blocks, mt, nt) == (-(-B * HW // 64), 64, 1) and slots * B * 2 <= st.numel(), list(a.out)
    out = dst.cpu().numpy()
    assert np.isnan(out[B * HW:]).all(), "a row past M was written"
    return out[:B * HW].reshape(B, HW, N), st[:B * slots * 2].cpu().numpy().reshape(B, slots, 2)


def per_layer(c):
    """the same layers one by one through spdm_op_gemm (the existing path): raw output of the last layer"""
    n, B, HW = len(c["chan"]) - 1, c["B"], c["HW"]
    cur, st = torch.from_numpy(c["x"]), None
    for i in range(n):
        K, N = c["chan"][i], c["chan"][i + 1]
        w9 = torch.zeros(N, K, 3, 3)
        w9[:, :, :, 1] = torch.from_numpy(c["w"][i]).permute(1, 2, 0)
        kw = {}
        pro = G.PRO_NONE
        if i:
            pro = G.PRO_GN_GELU if c["gelus"][i] else G.PRO_GN
            kw = dict(src_st=st, gamma=torch.from_numpy(c["gamma"][i]), beta=torch.from_numpy(c["beta"][i]))
        r = G.op_gemm(B, HW, 1, K, N, 3, 1, pro, G.EPI_STATS, cur, w9, **kw)
        cur, st = r["out"], (r["stats"], r["slots"], r["st_m"], r["st_n"], N)
    return cur.numpy()


def check_stats(out, st, tag):
    want = R.sums(out.astype(np.float64))
    n = out.shape[1] * out.shape[2]
    assert np.isfinite(st[:, 0]).all(), tag
    mean, var = want[:, 0] / n, want[:, 1] / n - (want[:, 0] / n) ** 2
    m1, v1 = st[:, 0, 0] / n, st[:, 0, 1] / n - (st[:, 0, 0] / n) ** 2
    assert float((np.abs(m1 - mean) / np.sqrt(np.maximum(var, 1e-30))).max()) <= 1e-6, (tag, "mean")
    assert float((np.abs(v1 - var) / np.maximum(var, 1e-30)).max()) <= 1e-5, (tag, "variance")


@pytest.mark.parametrize("HW,B", SHAPES, ids=[f"HW{h}-B{b}" for h, b in SHAPES])
@pytest.mark.parametrize("name", list(LISTS))
def test_fused_against_float64_and_the_per_layer_path(name, HW, B):
    c = make_case(LISTS[name], HW, B)
    want = R.chain(c["x"], c["w"], c["gamma"], c["beta"], c["gelus"])[-1]
    scale = np.abs(want).max()
    fused, st = op_chain(c)
    assert np.isfinite(fused).all()
    e_fused = float(np.abs(fused - want).max() / scale)
    e_layer = float(np.abs(per_layer(c) - want).max() / scale)
    print(f"TAU {name}-HW{HW}-B{B} fused {e_fused:.3e} per-layer {e_layer:.3e}")
    check_stats(fused, st, (name, HW, B))
    assert e_fused <= 2.0 * e_layer, (name, HW, B, e_fused, e_layer)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("name,HW,B", [("down3", 4, 33), ("down3", 4, 20), ("narrow", 8, 9)])
def test_no_tap_crosses_a_sample_and_no_row_past_m_counts(name, HW, B):
    c = make_case(LISTS[name], HW, B, seed=3)
    base, st0 = op_chain(c)
    for s in (0, B // 2, B - 1):
        x = c["x"].copy()
        x[s] *= 100.0
        got, st = op_chain(c, x)
        others = np.arange(B) != s
        assert np.isfinite(got).all()
        assert (_bits(got[others]) == _bits(base[others])).all(), f"sample {s}: another sample's output moved"
        assert (_bits(st[others, 0]) == _bits(st0[others, 0])).all(), f"sample {s}: another sample's statistics moved"
        assert not (_bits(got[s]) == _bits(base[s])).all()


def test_two_launches_equal_bits():
    for name, HW, B in (("bot", 4, 20), ("narrow", 8, 9)):
        c = make_case(LISTS[name], HW, B, seed=5)
        a, sa = op_chain(c)
        b, sb = op_chain(c)
        assert (_bits(a) == _bits(b)).all() and (_bits(sa[:, 0]) == _bits(sb[:, 0])).all()


def test_recorded_tau_file_lists_every_case():
    with open(os.path.join(ROOT, "tests", "golden", "conv_chain_tau.json")) as fh:
        rec = json.load(fh)["cases"]
    for name in LISTS:
        for HW, B in SHAPES:
            r = rec[f"{name}-HW{HW}-B{B}"]
            assert r["fused"] <= 2.0 * r["per_layer"], (name, HW, B, r)


# ---- the whole model, in fresh processes (the knob is read once) ------------------------------------------------------------
MODEL_CASES = [(20, 32, 3), (9, 64, 6)]      # (B, H, D)
REFUSED = (5, 16, 3)                         # the coarsest map is 2 x 1: samples of 2 rows, below the shape rule's HW >= 4
CD = 33

_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import test_gpu_conv_chain as T
np.savez(sys.argv[2], **T.child_run())
"""


def _inputs(B, H, D):
    g = torch.Generator().manual_seed(H * 7 + B)
    return (torch.randn(B, 1, H, D, generator=g), torch.randn(B, 1, 3, 11, generator=g), (torch.arange(B) * 29) % 1000)


def child_run():
    from state_policy_diffusionmodel_amd import _lib
    from state_policy_diffusionmodel_amd.schedulers import DDPMScheduler
    from test_gpu_parity import make_engine, weights
    lib = _lib.load()
    sd = weights(CD, 21)
    out = {}
    for tag, (B, H, D), debug in ([(f"m{i}", s, False) for i, s in enumerate(MODEL_CASES)] + [("refused", REFUSED, False), ("debug", MODEL_CASES[0], True)]):
        x, y, t = _inputs(B, H, D)
        eng = make_engine(H, D, CD, B, sd, debug=debug)
        try:
            n0 = lib.spdm_debug_conv_chain_launches()
            out[tag] = eng.unet_forward(x.cuda(), t, y.cuda()).cpu().numpy()
            n1 = lib.spdm_debug_conv_chain_launches()
            eng.unet_forward(x.cuda(), t, y.cuda())
            out[tag + "_rise"] = np.array([n1 - n0, lib.spdm_debug_conv_chain_launches() - n1])
            out[tag + "_routes"] = np.array(eng.plan_routes(B)["chain"])
            assert not eng.nonfinite()
        finally:
            eng.close()
    # a 4-step sampling loop, replayed as a hipGraph and with plain launches
    B, H, D = MODEL_CASES[0]
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(B, 1, 3, 11, generator=g).cuda()
    x_T = torch.rand(B, 1, H, D, generator=g).cuda()
    inpaint = (torch.rand(B, 1, 1, D, generator=g) * 2 - 1).cuda()
    eng = make_engine(H, D, CD, B, sd, T=4)
    try:
        sched = DDPMScheduler(num_train_timesteps=4)
        sched.set_timesteps(4)
        eng.set_scheduler(sched)
        for mode in ("graph", "plain"):
            eng.set_switch("SPDM_NO_GRAPH", mode == "plain")
            n0 = lib.spdm_debug_conv_chain_launches()
            x0, hist = eng.sample(cond, x_T, noise=None, inpaint=inpaint, seed=3, history=True)
            out["loop_" + mode] = hist.cpu().numpy()
            out["loop_" + mode + "_rise"] = np.array([lib.spdm_debug_conv_chain_launches() - n0])
    finally:
        eng.close()
    return out


@pytest.fixture(scope="module")
def model_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("conv_chain")
    procs = {}
    for knob in (7, 0):
        env = {k: v for k, v in os.environ.items() if k != KNOB}
        env[KNOB] = str(knob)
        out = d / f"knob{knob}.npz"
        procs[knob] = (subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, str(out)], env=env, stdout=subprocess.PIPE,
                                        stderr=subprocess.PIPE, text=True), out)
    got = {}
    try:
        for knob, (p, out) in procs.items():
            _, err = p.communicate(timeout=600)
            assert p.returncode == 0, (knob, err[-3000:])
            got[knob] = dict(np.load(out))
    finally:
        for p, _ in procs.values():          # trouble ends the step: no child keeps the GPU open
            if p.poll() is None:
                p.kill()
                p.communicate()
    return got


def test_whole_model_with_the_route_forced(model_runs):
    from oracle.unet_film_ref import unet_film_forward
    from test_gpu_parity import weights
    on, off = model_runs[7], model_runs[0]
    sd = weights(CD, 21)
    for i, (B, H, D) in enumerate(MODEL_CASES):
        x, y, t = _inputs(B, H, D)
        want = unet_film_forward(sd, x, t, y).numpy()
        err = float(np.abs(on[f"m{i}"] - want).max())
        print(f"whole model B{B} H{H} D{D}: max |eps - oracle| fused {err:.3e}, per-layer {float(np.abs(off[f'm{i}'] - want).max()):.3e}, "
              f"max |fused - per-layer| {float(np.abs(on[f'm{i}'] - off[f'm{i}']).max()):.3e}")
        assert err <= TOL, (B, H, D, err)
        assert on[f"m{i}_rise"].tolist() == [2, 2] and on[f"m{i}_routes"].tolist() == [1, 1], (on[f"m{i}_rise"], on[f"m{i}_routes"])
        assert off[f"m{i}_rise"].tolist() == [0, 0] and off[f"m{i}_routes"].tolist() == [0, 0]


@pytest.mark.parametrize("tag", ["refused", "debug"])
def test_route_not_taken_keeps_the_parent_path_bits(model_runs, tag):
    on, off = model_runs[7], model_runs[0]
    assert on[tag + "_rise"].tolist() == [0, 0] and on[tag + "_routes"].tolist() == [0, 0], (on[tag + "_rise"], on[tag + "_routes"])
    assert off[tag + "_rise"].tolist() == [0, 0]
    assert (_bits(on[tag]) == _bits(off[tag])).all()


def test_graph_replay_equals_plain_launches_with_the_route_forced(model_runs):
    on = model_runs[7]
    assert on["loop_graph"].shape[0] == 5
    assert (_bits(on["loop_graph"]) == _bits(on["loop_plain"])).all()
    assert on["loop_plain_rise"][0] == 2 * 4                    # plain launches: two per step
    assert 2 <= on["loop_graph_rise"][0] <= 2 * 4               # a captured step counts once, not per replay
