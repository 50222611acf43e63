"""Every reduction, geometry and branch kernel of the training pass, one launch at a time (spdm_op_train), against the plain
float64 CPU reference of tests/train_ops_ref.py on data the test controls.

Tolerance, per element and with no element left out: |got - ref64| <= TAU * S.  S is the same expression with every term in
absolute value; TAU = 4 x the worst error, in units of S, of the float32 reference that takes every sum sequentially -- computed
from the references alone by train_ops_ref.tau (tests/golden/train_ops_tau.json holds the values), never from the device.
Where S is zero (padded lanes, side columns, zero gradients, copies, the pooling gather's one add) the bound is equality.
Every output buffer is filled with NaN before the launch, so an element the kernel does not write fails.  Every case runs
twice and must give the same bits, and asserts from info[] the chunk or block geometry it is meant to hit.

Worst measured ratio of error to bound per op over its cases (MI355X, first run; seeded data, deterministic kernels); 'unit'
covers every shape on randn data, 'flavours' the offsets / ties / peaked / extremes / large data of the op:
    op                cases   unit    flavours
    wgrad               9     0.25    0.05  (large)
    wgrad_mapped        4     0.24    -
    colsum              7     0.26    -
    gn_stats           35     0.07    0.05  (offsets)
    gn_bwd             20     0.16    0.13  (offsets)
    gn_bwd_mapped      15     0.14    0.14  (offsets)
    film_bwd           11     0.25    -
    mse                 5     0.25    -
    pool_bwd            7     0 (equality)
    up_bwd              6     0.25    -
    mish_bwd            5     0.08    0.10  (extremes)
    silu_bwd            5     0.25    0.18  (extremes)
    gelu_bwd            7     0.18    0.18  (extremes)
    ln_fwd             15     0.12    0.09  (offsets)
    ln_bwd             16     0.25    0.25  (offsets)
    attn_fwd_lse       14     0.23    0.16  (peaked)
    attn_bwd           15     0.23    0.17  (peaked)
    simple_tail_bwd     5     0.32    -
The many ratios of exactly 0.25 are sums of a few terms (HW = 4 or 5 rows, three samples) that the kernel adds in the very
order of the sequential reference: its error is then the reference's own, a quarter of the bound.  simple_tail_bwd's 0.32 is
its four row lanes added pairwise-in-order where the reference adds five rows in sequence.
A first version of the peaked data put the +1000 score offset in the LAST coordinate of q and k.  attn_bwd then measured
2.8 (L 4, d 64), 1.6 and 1.2: a sequential sum meets the offset last and rounds at that magnitude once, while the kernel's
four partial sums round there three times -- the sequential order was the best, not the worst, for that row.  The kernel's
error (|s| u times a few) is what float32 scores of 1000 cost; the data now carry the offset in coordinate 0, where the
sequential reference rounds at 1000 in every later addition, and TAU follows it.
"""
import ctypes

import numpy as np
import pytest
import torch

import train_ops_ref as R

pytestmark = pytest.mark.gpu

ALL = [(op, case) for op in R.OPS for case in R.cases(op)]
IDS = [f"{op}-{case[0]}" for op, case in ALL]


def _lib():
    from state_policy_diffusionmodel_amd import _lib as L
    return L, L.load()


def op_train(op, inp):
    """One launch of a case: ({output name: float64 array}, info, {output name: raw bytes})."""
    L, lib = _lib()
    dims, bufs, idx, outs = R.launch_plan(op, inp)
    a = L.SpdmOpTrainArgs()
    a.op = L.OP_TRAIN_OPS.index(op)
    for i, v in enumerate(dims):
        a.dim[i] = v
    dev = []
    for i, b in enumerate(bufs):
        if b is None:
            dev.append(None)
            continue
        if b[0] == "out":
            t = torch.full((b[1],), float("nan"), dtype=torch.float32, device="cuda")
        else:
            t = torch.from_numpy(np.ascontiguousarray(b[1], np.float32).reshape(-1)).cuda()
        dev.append(t)
        a.d_buf[i], a.cap[i] = t.data_ptr(), t.numel()
    keep = []
    for k, arr in enumerate(idx):
        keep.append(arr)
        a.h_idx[k], a.n_idx[k] = arr.ctypes.data, arr.size
    torch.cuda.synchronize()
    L.check(lib.spdm_op_train(ctypes.byref(a)), f"spdm_op_train({op})")
    got, raw = {}, {}
    for name, (i, shape, stride) in outs.items():
        flat = dev[i].cpu().numpy()
        raw[name] = flat.tobytes()
        if stride is None:
            got[name] = flat.reshape(shape).astype(np.float64)
        else:                                                                  # rows of `stride` floats, shape[1] written per row
            written = np.arange(flat.size) % stride < shape[1]
            got[name] = flat[written].reshape(shape).astype(np.float64)
            assert np.isnan(flat[~written]).all(), f"{name}: the launch wrote between the rows"
    return got, list(a.info), raw


@pytest.mark.parametrize("op,case", ALL, ids=IDS)
def test_launch_against_fp64(op, case):
    inp = R.make_inputs(op, case)
    ref, scale = R.ref64(op, inp), R.scale64(op, inp)
    tau = R.tau(op, inp, ref, scale)
    got, info, raw = op_train(op, inp)
    assert set(got) == set(ref)
    ratio = R.worst_ratio(got, ref, scale, tau)
    print(f"RATIO {op} {case[0]} {ratio:.4f} (tau {tau / R.U:.2f} u)")
    want_info = R.expected_info(op, inp)
    if want_info is not None:                                                  # the edge the case is meant to hit
        assert tuple(info[:len(want_info)]) == tuple(want_info), (info, want_info)
        if "geom" in case[1]:
            assert tuple(info[:2]) == case[1]["geom"]
    for name, v in got.items():
        assert np.isfinite(v).all(), f"{name}: not finite"
    assert ratio <= 1.0, f"{op} {case[0]}: error / (TAU S) = {ratio:.3f}"
    again = op_train(op, inp)[2]
    assert again == raw, "two launches on the same inputs differ"
