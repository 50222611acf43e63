"""Every streaming kernel of the forward / sampling path (csrc/elementwise.hip), one launch at a time (spdm_op_stream), against
the plain float64 CPU reference of tests/stream_ops_ref.py on data the test controls.

Tolerance, per element and with no element left out: |got - ref64| <= TAU * S.  S is the same expression with every term in
absolute value; TAU = 4 x the worst error, in units of S, of the float32 reference that takes every sum sequentially, floored
by a count of roundings for the ops with math-library calls -- computed from the references alone by stream_ops_ref.tau
(tests/golden/stream_ops_tau.json holds the values), never from the device.  Where S is zero (padded lanes, copied channels,
zero-padded columns, a MaxPool with no GroupNorm, the step and t words, outputs no data reaches) the bound is equality.
Every output buffer -- floats, doubles and the words -- is filled with NaN (the words with a poison value) before the launch,
so an element the kernel does not write fails, and a statistics slot it should not write must still be NaN afterwards.  A
pending GroupNorm's unused partial slots are NaN, so a consumer that reads one slot too many fails.  Every case runs twice and
must give the same bits, and asserts from info[] the geometry it is meant to hit.

Worst measured ratio of error to bound per op over its cases (MI355X, first run; seeded data, deterministic kernels); 'unit'
covers every shape on randn data, 'flavours' the offset / constant / ties / ladder / cancelling / non-finite data of the op:
    op                cases   unit    flavours
    conv_in            19     0.27    0.15  (mean 10)
    pool               45     0.23    0.25  (mean -300)
    upcat              51     0.29    0.50  (constant, clamped variance)
    film_apply         27     0.24    0.34  (constant)
    film_coef          27     0.25    0.24  (constant)
    layernorm          24     0.13    0.05  (mean -300)
    mish_pad            6     0.20    0.18  (ladder)
    silu_pad            6     0.19    0.23  (ladder)
    silu                6     0.20    0.16  (ladder)
    dc_finish          17     0.07    0.06  (mean 10)
    simple_tail        23     0.08    0.04  (ladder)
    splitk_combine     19     0.25    0.25  (cancelling slabs)
    out_step           27     0.10    0.08  (non-finite features; eps and the Philox normal -- every other element is equal)
The ratios of 0.25 are short sums the kernel adds in the sequential reference's own order: its error is the reference's own,
a quarter of the bound.  upcat's 0.50 is a constant source whose (v - mu) is exactly zero: S is (|v| + |mu|) rstd |gamma| = 6e3 |gamma| while the
output is beta, the float32 reference is off by half an ulp of beta in one element, TAU S is four times that, and the kernel's
blend of four equal values is off by one ulp.
One finding, a kernel bug: out_step's full step from a given eps first failed its EQUALITY in 11 of 27 cases (every case not
overwritten whole by the in-painting rows; 2 of 144 elements one ulp off at the last DDPM step).  hipcc's __fmul_rn / __fsub_rn
are plain operators in an inline header function under -ffp-contract=fast, and x - c0 * eps had become one FMA; of the variants
tried only `fma / div / add(mul, mul)` matched every element.  elementwise.hip now rounds each operation by itself
(mul_rn / sub_rn / add_rn with contraction off) and all 27 cases are equal; DESIGN.md 8.16.
"""
import ctypes

import numpy as np
import pytest
import torch

import stream_ops_ref as R

pytestmark = pytest.mark.gpu

ALL = [(op, case) for op in R.OPS for case in R.cases(op)]
IDS = [f"{op}-{case[0]}" for op, case in ALL]
POISON = -0x5A5A5A5A


def _lib():
    from state_policy_diffusionmodel_amd import _lib as L
    return L, L.load()


def op_stream(op, inp):
    """One launch of a case: ({output name: float64 array}, info, {output name: raw bytes})."""
    L, lib = _lib()
    P = R.launch_plan(op, inp)
    a = L.SpdmOpStreamArgs()
    a.op = L.OP_STREAM_OPS.index(op)
    for i, v in enumerate(P["dims"]):
        a.dim[i] = v
    dev, keep = {}, []
    for i, b in enumerate(P["bufs"]):
        if b is None:
            continue
        if b[0] == "out":
            t = torch.full((b[1],), float("nan"), dtype=torch.float32, device="cuda")
        else:
            t = torch.from_numpy(np.ascontiguousarray(b[1], np.float32).reshape(-1)).cuda()
        dev[i] = t
        a.d_buf[i], a.cap[i] = t.data_ptr(), t.numel()
    if P["idx"] is not None:
        a.h_idx[0], a.n_idx[0] = P["idx"].ctypes.data, P["idx"].size
    for k, g in enumerate(P["gn"]):
        if g is None:
            continue
        st = torch.from_numpy(np.ascontiguousarray(g["stats"], np.float64).reshape(-1)).cuda()
        ga, be = (torch.from_numpy(np.ascontiguousarray(g[n], np.float32)).cuda() for n in ("gamma", "beta"))
        keep += [st, ga, be]
        a.gn[k].d_stats, a.gn[k].stats_cap = st.data_ptr(), st.numel()
        a.gn[k].slots, a.gn[k].m_tile, a.gn[k].n_tiles, a.gn[k].cnorm = g["slots"], g["m_tile"], g["n_tiles"], g["cnorm"]
        a.gn[k].d_gamma, a.gn[k].d_beta, a.gn[k].affine_cap = ga.data_ptr(), be.data_ptr(), ga.numel()
    if P["stats_out"] is not None:
        dev["stats"] = torch.full((P["stats_out"],), float("nan"), dtype=torch.float64, device="cuda")
        a.d_stats_out, a.stats_out_cap = dev["stats"].data_ptr(), dev["stats"].numel()
    if P["words"]:
        dev["words"] = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
        a.d_words = dev["words"].data_ptr()
    a.bias, a.seed, a.first_index = P.get("bias", 0.0), P.get("seed", 0), P.get("first", 0)
    torch.cuda.synchronize()
    rc = lib.spdm_op_stream(ctypes.byref(a))
    if rc not in (0, L.SPDM_ERR_INVALID):                                      # a device error: nothing more is launched on it
        pytest.exit(f"spdm_op_stream({op}) failed ({rc}): {lib.spdm_last_error().decode()}", returncode=3)
    L.check(rc, f"spdm_op_stream({op})")
    got, raw = {}, {}
    for name, (src, shape, stride) in P["outs"].items():
        flat = dev["words" if src == "flag" else src].cpu().numpy()
        raw[name] = flat.tobytes()
        if src in ("words", "flag"):                                           # {step, t} of the bookkeeping; the non-finite flag
            flat = flat[:2] if src == "words" else flat[2:]
        if stride is None:
            got[name] = flat.reshape(shape).astype(np.float64)
        else:                                                                  # rows of `stride` elements, the first ones written
            written = np.arange(flat.size) % stride < int(np.prod(shape[1:]))
            got[name] = flat[written].reshape(shape).astype(np.float64)
            assert np.isnan(flat[~written]).all(), f"{name}: the launch wrote between the rows"
    return R.finish_got(op, got), list(a.info), raw


def _eps_of_the_same_launch(op, inp):
    """out_step from the features: the eps its eps-only mode stores on the same inputs -- itself held to float64 under the bound
    -- is what the full step must equal the float32 restatement on."""
    inp0 = {**inp, "mode": 0}
    ref, scale = R.ref64(op, inp0), R.scale64(op, inp0)
    got, _, raw = op_stream(op, inp0)
    ratio = R.worst_ratio(got, ref, scale, R.tau(op, inp0, ref, scale))
    assert ratio <= 1.0, f"eps-only mode of the same launch: error / (TAU S) = {ratio:.3f}"
    return np.frombuffer(raw["eps"], np.float32).reshape(ref["eps"].shape).copy()


@pytest.mark.parametrize("op,case", ALL, ids=IDS)
def test_launch_against_fp64(op, case):
    inp = R.make_inputs(op, case)
    if op == "out_step" and inp["mode"] == 1:
        inp["eps_dev"] = _eps_of_the_same_launch(op, inp)
    ref, scale = R.ref64(op, inp), R.scale64(op, inp)
    tau = R.tau(op, inp, ref, scale)
    got, info, raw = op_stream(op, inp)
    assert set(got) == set(ref)
    ratio = R.worst_ratio(got, ref, scale, tau)
    print(f"RATIO {op} {case[0]} {ratio:.4f} (tau {tau / R.U:.2f} u)")
    want_info = R.expected_info(op, inp)
    if want_info is not None:                                                  # the edge the case is meant to hit
        assert tuple(info[:len(want_info)]) == tuple(want_info), (info, want_info)
        assert info[0] == (case[1]["parts"] if op == "conv_in" else R.combine_rows(case[1]["HW"], case[1]["N"]))
    for name, v in got.items():
        assert np.isfinite(v).all(), f"{name}: not finite"
    assert ratio <= 1.0, f"{op} {case[0]}: error / (TAU S) = {ratio:.3f}"
    again = op_stream(op, inp)[2]
    assert again == raw, "two launches on the same inputs differ"
