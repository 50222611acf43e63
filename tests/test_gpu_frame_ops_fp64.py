"""Every kernel of the observation encoder and of the autoencoder's decoder (csrc/encoder.hip, encoder_train.hip, decoder.hip),
one launch at a time (spdm_op_frame), against the plain float64 CPU reference of tests/frame_ops_ref.py on data the test controls:
torch's default initialisation as a control, trained-scale weights (saturated sigmoid, 8-bit frames, recon - target cancelling),
dead ReLU channels and whole dead layers, z6 beyond +-104, all-black / all-white frames, saved activations at +0.0, -0.0, the
smallest normal and a subnormal.

Tolerance, per element and with no element left out: |got - ref64| <= TAU * S, TAU = 4 x the worst error, in units of S, of the
float32 reference that takes every sum sequentially (tests/golden/frame_ops_tau.json), never from the device; where S is zero the
bound is equality.  The kink kernels, the masked and the layout permutations and ADD must give the reference's bits.  `sq` is held
to the float64 formula on the device's own float32 reconstruction, `loss` to the float64 formula on the given sums.  The two
variants of each forward kernel must give the same bits; every output buffer is NaN before the launch; every case runs twice
(equal bits) and asserts its geometry from info[].

Worst measured error / bound per op over its cases (MI355X, first run; the last test prints them):
    op                cases   worst
    enc_convs          12     0.36
    enc_kinks          17     bits
    enc_x2              5     0.25
    enc_dz3, enc_dz2   9 + 9  bits
    enc_conv1_wgrad     9     0.26
    add                 4     bits
    dec_convs          14     0.27   (sq, 7 cases: 0.25)
    dec_kinks          17     bits
    dec_loss            6     0.25
    dec_bwd6           10     0.10
    dec_dgrad4          9     0.30
    dec_colsum         21     0.25
    dec_unperm_*       3 + 1  bits
    frame_wgrad        24     0.29
The ratios of 0.25 are short sums the kernel adds in the reference's own order, and `sq` / `loss`, whose model takes the kernel's
own float32 difference and float32 store.  No kernel had to change.
"""
import ctypes

import numpy as np
import pytest
import torch

import frame_ops_ref as R

pytestmark = pytest.mark.gpu

ALL = [(op, case) for op in R.OPS for case in R.cases(op)]
IDS = [f"{op}-{case[0]}" for op, case in ALL]
WORST = {}


def _lib():
    from state_policy_diffusionmodel_amd import _lib as L
    return L, L.load()


def op_frame(op, inp):
    """One launch of a case: ({output name: float32 array}, info, {output name: raw bytes}, sq or None)."""
    L, lib = _lib()
    dims, bufs, outs = R.launch_plan(op, inp)
    a = L.SpdmOpFrameArgs()
    a.op = L.OP_FRAME_OPS.index(op)
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
            t = torch.from_numpy(np.ascontiguousarray(b[1], np.float32).reshape(-1).copy()).cuda()
        dev.append(t)
        a.d_buf[i], a.cap[i] = t.data_ptr(), t.numel()
    sq = None
    if op == "dec_loss":
        sq = torch.from_numpy(np.ascontiguousarray(inp["sq"], np.float64)).cuda()
    elif op == "dec_convs" and inp["train"]:
        sq = torch.full((inp["n"],), float("nan"), dtype=torch.float64, device="cuda")
    if sq is not None:
        a.d_sq, a.sq_cap = sq.data_ptr(), sq.numel()
    if op == "dec_bwd6":
        a.scale = inp["scale"]
    torch.cuda.synchronize()
    rc = lib.spdm_op_frame(ctypes.byref(a))
    if rc == -2:                                                               # a device error: nothing after it can be trusted
        pytest.exit(f"spdm_op_frame({op}) failed ({rc}): {lib.spdm_last_error().decode()}", returncode=3)
    L.check(rc, f"spdm_op_frame({op})")
    got, raw = {}, {}
    for name, (i, shape) in outs.items():
        flat = dev[i].cpu().numpy()
        raw[name] = flat.tobytes()
        got[name] = flat.reshape(shape)
    if op == "dec_convs" and inp["train"]:
        raw["sq"] = sq.cpu().numpy().tobytes()
    return got, list(a.info), raw, (None if sq is None else sq.cpu().numpy())


@pytest.mark.parametrize("op,case", ALL, ids=IDS)
def test_launch_against_fp64(op, case):
    inp = R.make_inputs(op, case)
    ref, scale = R.ref64(op, inp), R.scale64(op, inp)
    tau = R.tau(op, inp, ref, scale)
    got, info, raw, sq = op_frame(op, inp)
    assert set(got) == set(ref)
    ratio = R.worst_ratio(got, ref, scale, tau)
    print(f"RATIO {op} {case[0]} {ratio:.4f} (tau {tau / R.U:.2f} u)")
    WORST[op] = max(WORST.get(op, 0.0), ratio)
    want_info = R.expected_info(op, inp)
    if want_info is not None:                                                  # the edge the case is meant to hit
        assert tuple(info[:len(want_info)]) == tuple(want_info), (info, want_info)
    for name, v in got.items():
        assert np.isfinite(v).all(), f"{name}: not finite"
    assert ratio <= 1.0, f"{op} {case[0]}: error / (TAU S) = {ratio:.3f}"
    if op in R.EXACT:                                                          # the reference's bits, -0.0 and subnormals included
        for name, v in R.exact32(op, inp).items():
            assert raw[name] == np.ascontiguousarray(v, np.float32).tobytes(), f"{op} {case[0]}: {name} differs in bits"
    if op == "enc_x2":                                                         # on: never below the smallest normal; off: exactly 0
        on = ref["x2"] > 0
        assert (got["x2"][on] >= R.KINK).all() and not got["x2"][~on].any()
    if op in ("enc_convs", "dec_convs") and inp["train"]:                      # the training variant is the forward's arithmetic
        name = "feat" if op == "enc_convs" else "recon"
        assert op_frame(op, dict(inp, train=0))[2][name] == raw[name], f"{name}: the two variants differ in bits"
    if op == "dec_convs" and inp["train"]:                                     # float64 on the device's own float32 reconstruction
        r64, S, model = R.sq_refs(got["recon"], inp["target"])
        t = R.sq_tau(r64, S, model)
        worst = float((np.abs(sq - r64) / (t * S)).max())
        print(f"RATIO dec_convs_sq {case[0]} {worst:.4f} (tau {t:.3e})")
        WORST["dec_convs_sq"] = max(WORST.get("dec_convs_sq", 0.0), worst)
        assert np.isfinite(sq).all() and worst <= 1.0, f"sq: error / (TAU S) = {worst:.3f}"
    again = op_frame(op, inp)[2]
    assert again == raw, "two launches on the same inputs differ"


def test_print_worst_ratio_per_op():
    for op in sorted(WORST):
        print(f"WORST {op} {WORST[op]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
