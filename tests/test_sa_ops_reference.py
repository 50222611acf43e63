"""tests/sa_ops_ref.py held on the CPU, before tests/test_gpu_sa_ops_fp64.py holds the HIP kernels to it:
  1. the references against float64 torch (F.layer_norm, F.scaled_dot_product_attention, F.linear, F.gelu) to 1e-12 of S;
  2. THE ADMISSION CONDITION: a plain float32 CPU evaluation of every case lies within 0.5 of the case's bound on every element.
     This is what keeps the GPU test from failing on conditioning rather than on a kernel -- data that float32 itself cannot
     carry to half the bound is not a test of a float32 kernel;
  3. every mutant violates the bound in some case of its op;
  4. tests/golden/sa_ops_tau.json holds the TAU_op the two restatements produce here (never a device), and a TAU_op is no
     blanket: both restatements are within a quarter of it and it stays far below anything that would pass a wrong kernel.
"""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sa_ops_ref as R

ALL = [(op, case) for op in R.OPS for case in R.cases(op)]
_CACHE = {}


def case_data(op, case):
    key = (op, case[0])
    if key not in _CACHE:
        inp = R.make_inputs(op, case)
        if inp.get("refused"):
            _CACHE[key] = (inp, None, None, None)
        else:
            ref = R.ref64(op, inp)
            tau = None if op == "fused64" else R.tau(op, inp, ref)
            _CACHE[key] = (inp, ref, R.bound(op, inp, tau), tau)
    return _CACHE[key]


def _torch_block(W, xa, C):
    """the block from torch.nn.functional alone, float64: (qkv, att, out) channels-last"""
    w = {k: torch.from_numpy(v).double() for k, v in W.items()}
    x = torch.from_numpy(xa)
    B, L, _ = x.shape
    qkv = F.linear(F.layer_norm(x, (C,), w["ln.weight"], w["ln.bias"], 1e-5), w["attention.in_proj_weight"], w["attention.in_proj_bias"])
    hd = lambda z: z.reshape(B, L, R.HEADS, C // R.HEADS).transpose(1, 2)
    q, k, v = (hd(z) for z in qkv.split(C, -1))
    att = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, C)
    a = F.linear(att, w["attention.out_proj.weight"], w["attention.out_proj.bias"]) + x
    f = F.linear(F.layer_norm(a, (C,), w["ff_self.0.weight"], w["ff_self.0.bias"], 1e-5), w["ff_self.1.weight"], w["ff_self.1.bias"])
    out = F.linear(F.gelu(f), w["ff_self.3.weight"], w["ff_self.3.bias"]) + a
    return qkv.numpy(), att.numpy(), out.numpy()


@pytest.mark.parametrize("op", R.OPS)
def test_ref64_is_torch_in_float64(op):
    for case in R.cases(op):
        inp, ref, bd, tau = case_data(op, case)
        if ref is None:
            continue
        C, sub = inp["C"], R.subset(inp)
        if op == "core":
            qkv = torch.from_numpy(inp["qkv"][sub]).double()
            B, L = qkv.shape[:2]
            hd = lambda z: z.reshape(B, L, R.HEADS, C // R.HEADS).transpose(1, 2)
            want = F.scaled_dot_product_attention(*(hd(z) for z in qkv.split(C, -1))).transpose(1, 2).reshape(B, L, C).numpy()
            s = R.scale64(op, inp)["out"]
        else:
            ab = R.coefficients(inp)
            xa = R._affine(R.N64(), inp["x"][sub].astype(np.float64), None if ab is None else ab[sub])
            qkv, att, out = _torch_block(inp["W"], xa, C)
            if op == "tail":                                                       # from the given head outputs
                w = {k: torch.from_numpy(v).double() for k, v in inp["W"].items()}
                a = F.linear(torch.from_numpy(inp["att"][sub]).double(), w["attention.out_proj.weight"], w["attention.out_proj.bias"]) + torch.from_numpy(xa)
                f = F.linear(F.layer_norm(a, (C,), w["ff_self.0.weight"], w["ff_self.0.bias"], 1e-5), w["ff_self.1.weight"], w["ff_self.1.bias"])
                out = (F.linear(F.gelu(f), w["ff_self.3.weight"], w["ff_self.3.bias"]) + a).numpy()
            want = {"qkv": qkv, "head": att, "tail": out, "fused64": out}[op]
            s = np.abs(want) + 1 if op == "fused64" else R.scale64(op, inp)["out"]
            if op == "fused64" and inp.get("crop"):
                c = inp["crop"]
                tok = [(c["lh"] + i) * c["Wp"] + c["lw"] + j for i in range(c["H0"]) for j in range(c["D"])]
                want, s = want[:, tok], s[:, tok]
                if inp.get("outc"):
                    want = (want @ inp["outc"][0].astype(np.float64) + inp["outc"][1]).reshape(len(sub), c["H0"], c["D"])
                    s = np.abs(want) + 1
        got = ref["eps" if op == "fused64" and inp.get("outc") else "out"]
        assert np.abs(got - want).max() <= 1e-12 * s.max() and (np.abs(got - want) <= 1e-12 * np.maximum(s, s.max() * 1e-3)).all(), (op, case[0])
        # the restatement the mutants, ref32 and ref_split are written on is the same function
        if op != "core":
            kw = dict(att_in=inp["att"][sub]) if op == "tail" else dict(stop={"qkv": "qkv", "head": "att"}.get(op))
            mine = R._forward(R.N64(), inp["W"], inp["x"][sub], None if ab is None else ab[sub], **kw)
            full = {"qkv": qkv, "head": att, "tail": out, "fused64": out}[op] if op != "fused64" else _torch_block(inp["W"], xa, C)[2]
            assert np.abs(mine - full).max() <= 1e-12 * (np.abs(full).max() + 1), (op, case[0])


@pytest.mark.parametrize("op", R.OPS)
def test_float32_itself_is_well_inside_the_bound(op):
    """the admission condition (module docstring, 2): worst element of plain float32 / bound <= 0.5 for every case"""
    for case in R.cases(op):
        inp, ref, bd, tau = case_data(op, case)
        if ref is None:
            continue
        ratio = R.worst_ratio(R.plain32(op, inp), ref, bd)
        assert ratio <= R.ADMIT, (op, case[0], ratio)


def test_the_chains_are_admitted_too():
    for route, C in R.CHAINS:
        first, cid, inp = R.chain_inputs(route, C)
        blk = R._block64(inp, inp["x"], R.coefficients(inp))
        ab32 = R.coefficients(inp, np.float32)
        got = R._forward(R._T32(), inp["W"], inp["x"], ab32).astype(np.float64)
        assert (np.abs(got - blk["out"]) / blk["bound"]).max() <= R.ADMIT, (route, C)


@pytest.mark.parametrize("op", R.OPS)
def test_every_mutant_violates_the_bound(op):
    missed = set(R.MUTANTS[op])
    for case in R.cases(op):
        inp, ref, bd, tau = case_data(op, case)
        if ref is None:
            continue
        for m in sorted(missed):
            if R.worst_ratio(R.ref64(op, inp, mutant=m), ref, bd) > 1.0:
                missed.discard(m)
        if not missed:
            break
    assert not missed, (op, sorted(missed))


def test_the_mutants_asked_for_are_all_there():
    have = set().union(*R.MUTANTS.values())
    assert have >= {"ab_after_ln", "resid_raw_x", "t_of_sample0", "gn_neighbour", "crop_stride_D", "lh_ignored", "lw_ignored",
                    "qw_last_dropped", "outc_bias_dropped", "key_tail_unmasked", "walk_stuck", "last_tile_dropped",
                    "straddle_first_coef", "heads_swapped", "k_fp16", "q_fp16", "p_fp16", "v_fp16", "skip_rescale", "mask_finite"}


@pytest.mark.parametrize("op", [o for o in R.OPS if o != "fused64"])
def test_both_restatements_are_within_a_quarter_of_tau(op):
    for case in R.cases(op):
        inp, ref, bd, tau = case_data(op, case)
        if ref is None:
            continue
        s = {"out": tau * R.scale64(op, inp)["out"]}
        for f in (R.ref32, R.ref_split):
            assert R.worst_ratio(f(op, inp), ref, s) <= 1.0, (op, case[0], f.__name__)
        assert math.isfinite(tau) and R.FLOOR_U[op] * R.U <= tau < 1e-3, (op, case[0], tau)


def test_the_cases_reach_the_branches_they_are_written_for():
    fused = {c[0]: c[1] for c in R.cases("fused64")}
    assert {v["L"] for k, v in fused.items() if "crop" not in v and v["B"] == 3} >= {1, 5, 32, 35, 64, 128, 192, 256, 320, 512}
    assert {(v["L"], v["B"]) for v in fused.values()} >= {(128, 300), (256, 300)}
    crops = [v for v in fused.values() if v.get("crop")]
    assert {(v["crop"] + (v["L"],)) for v in crops} >= {(32, 3, 8, 0, 2, 256), (16, 3, 8, 0, 2, 128), (1, 1, 8, 3, 5, 64),
                                                        (32, 4, 8, 0, 0, 256), (16, 4, 8, 2, 3, 192)}
    assert any((v["crop"][0] * v["crop"][1]) % R.crop_waves(v["L"]) for v in crops)            # a Q that qw does not divide
    assert {v["L"] for v in crops} >= {35, 72} and {v["outc"] for v in crops} == {0, 1}
    for op in ("qkv", "tail"):
        for cid, v in R.cases(op):
            TM, rows = 8192 // v["C"], v["B"] * v["L"]
            assert v["L"] == 64 or (rows % 64 and rows % TM and rows > TM), (op, cid)           # more than one tile, the last ragged
            tiles = [(t, min(t + TM, rows)) for t in range(0, rows, TM)]                          # a tile that holds rows of two samples
            straddles = any(a // v["L"] != (b - 1) // v["L"] and (a % v["L"] or (b % v["L"] and b < rows)) for a, b in tiles)
            assert straddles == (TM % v["L"] != 0 and v["L"] % TM != 0), (op, cid)              # ... and cuts one of them
        for C in (128, 256):                                                                     # ... under per-sample coefficients
            assert {v["L"] for _, v in R.cases(op) if v["C"] == C and (8192 // C) % v["L"] and v.get("aff")} >= {3, 5, 20, 48, 80}
        assert {(v["C"], v["L"]) for _, v in R.cases(op)} >= {(C, L) for C in (128, 256) for L in (1, 3, 5, 16, 20, 48, 64, 80)}
    for C in (128, 256):
        TM = 8192 // C
        got = {(v["L"], v["B"]) for _, v in R.cases("head") if v["C"] == C}
        assert got >= {(L, B) for L in R.head_Ls(C) for B in (1, TM // L, TM // L + 1)}
    core = [v for _, v in R.cases("core")]
    assert {(v["C"] // 4, v["L"]) for v in core if not v["valu"] and v["L"] < 32} == {(d, L) for d in (16, 32, 64) for L in (1, 3, 4, 5, 12, 16, 20)}
    assert {(v["C"] // 4, v["L"]) for v in core if v["valu"]} == {(d, L) for d in (16, 32, 64) for L in (32, 48, 80)}
    assert all((v["B"] * 4) % (64 // v["L"]) for v in core if v["L"] in (1, 4))                 # npairs % G != 0 (G = 64 / L > 4)
    refused = [c[0] for c in R.cases("core") if R.make_inputs("core", c)["refused"]]
    assert refused == ["d64_L320_mfma", "d64_L512_mfma"]          # attention_mfma's own 160 KiB limit at d = 64 (csrc/attention.hip)


def test_a_whole_block_is_weakened_only_where_onehot_is_not_admitted():
    """'moderate' replaces 'onehot' only in the cases float32 itself does not carry on 'onehot' (above 128 tokens: not within
    0.45, sa_ops_ref.default_flavour); one 'plain' control; every other whole-block case runs on 'onehot'"""
    specs = dict(R.cases("fused64"))
    assert [k for k, v in specs.items() if v.get("flavour")] == ["L64_plain"]
    weak = {k for k, v in specs.items() if v.get("weak")}
    assert weak == {"L320", "L256_ab", "L256_film_t1", "L256_film_t3", "L128_B300", "L256_B300", "L35_amp3", "crop_h16_outc0",
                    "crop_h16_outc1"}
    for k in sorted(weak - {"crop_h16_outc1"}):                                  # (the outc twin shares crop_h16_outc0's weights)
        inp = R.make_inputs("fused64", (k, {**specs[k], "flavour": "onehot"}))
        ratio = R.worst_ratio(R.plain32("fused64", inp), R.ref64("fused64", inp), R.bound("fused64", inp))
        assert ratio > (0.45 if specs[k]["L"] > 128 else R.ADMIT), (k, ratio)
    assert all(R.default_flavour("fused64", v) == "onehot" for k, v in specs.items() if k not in weak)


def _table():
    return {f"{op}/{case[0]}": case_data(op, case)[3] / R.U for op, case in ALL if op != "fused64" and case_data(op, case)[1] is not None}


def test_the_golden_tau_table_is_current():
    """TAU_op of every partial-op case in units of u, as the references produce it here on the CPU (never from a device)"""
    want = json.load(open(R.GOLDEN))
    got = _table()
    assert set(got) == set(want)
    for k, v in got.items():
        assert abs(v - want[k]) <= 1e-6 * max(1.0, abs(want[k])), (k, v, want[k])
