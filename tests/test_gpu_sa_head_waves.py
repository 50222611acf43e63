"""sa_head_kernel with one head per wave, in registers (csrc/sa_tail.hip): what the mapping itself can get wrong.

After the LayerNorm slab, wave w forms q^T, k^T (weights as the A operand) and v of head w, keeps them as MFMA operands, and runs
S^T = k q^T, the softmax and O^T = v^T P^T without LDS or a barrier.  tests/test_gpu_sa_ops_fp64.py holds the launch against float64
on its own cases; here, through the same hook (spdm_op_sa, seeded data of tests/sa_ops_ref.py):

  head isolation     zeroed V rows and V bias of head h give exactly 0 in the columns of head h and the same bits everywhere else
                     (a wave <-> head or d-tile index slip moves another column);
  slot independence  the head output of a sample is the same bits wherever the sample sits in a tile, and alone (the mask and
                     the k-slot order of keys: the other samples' keys enter a query's sums as exact zeros);
  whole tile         one sample fills the tile: the only shapes without a masked key;
  L = 1              every token its own sample: the softmax of one key is exactly 1, the output is the token's v projection;
  ragged tile        rows beyond M are not written, rows below M are finite;
  old against new    SPDM_TUNE24 = 0 (the head-serial body) and 3 (this one) in fresh processes -- the knob is read once -- both
                     within the float64 bound; their difference is printed, not asserted (S and O accumulate in another order);
  determinism        two launches, equal bits.

Bounds: sa_ops_ref.bound('head', .) -- TAU_op S_op + the split format's floors, from the CPU restatements of the split arithmetic
alone -- on exactly the inputs of each case; nothing here is taken from what the kernel gives.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sa_ops_ref as R
import test_gpu_sa_ops_fp64 as OPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "SPDM_TUNE24"
IN_W, IN_B = "attention.in_proj_weight", "attention.in_proj_bias"
_KEEP = []                                                   # (op_sa keys its device vectors by the weight dict's id)


def _inputs(cid, C, B, L, **kw):
    return R.make_inputs("head", (cid, dict(C=C, B=B, L=L, data="alt3", **kw)))


def _head(inp, extra_rows=0):
    """one HEAD launch on the whole batch -> float32 [B L + extra_rows, C]; the buffer starts as NaN"""
    C, rows = inp["C"], inp["B"] * inp["L"]
    out = OPS._nan((rows + extra_rows) * C)
    info = OPS.op_sa("head", inp, bufs=(OPS._cuda(inp["x"]), out, None))
    assert (info["kernel"], info["waves"], info["grid"]) == ("head", 4, -(-rows // (8192 // C))), info
    return out.cpu().numpy().reshape(rows + extra_rows, C)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _ratio(got, inp):
    """worst |got - ref64| / bound over the compared samples (all of them up to B = 16)"""
    sub = R.subset(inp)
    g = got[: inp["B"] * inp["L"]].reshape(inp["B"], inp["L"], -1)[sub].astype(np.float64)
    return R.worst_ratio({"out": g}, R.ref64("head", inp), R.bound("head", inp))


@pytest.mark.parametrize("C,B", [(128, 5), (256, 3)])
def test_head_isolation(C, B):
    inp = _inputs(f"waves_iso_C{C}", C, B, 16)
    D = C // 4
    base = _head(inp)
    assert np.isfinite(base).all()
    for h in range(4):
        W = {k: v.copy() for k, v in inp["W"].items()}
        W[IN_W][2 * C + h * D: 2 * C + (h + 1) * D] = 0.0
        W[IN_B][2 * C + h * D: 2 * C + (h + 1) * D] = 0.0
        _KEEP.append(W)
        got = _head({**inp, "W": W})
        cols = np.arange(C) // D == h
        assert (got[:, cols] == 0.0).all(), f"head {h}: a column of the head with v = 0 is not 0"
        assert (_bits(got[:, ~cols]) == _bits(base[:, ~cols])).all(), f"head {h}: another head's column moved"


@pytest.mark.parametrize("C,B,L", [(128, 4, 16), (256, 8, 4)])
def test_slot_independence(C, B, L):
    inp = _inputs(f"waves_slot_C{C}", C, B, L)
    x = inp["x"]
    first = _head(inp)[:L]                                   # sample 0 in slot 0
    moved = {**inp, "x": np.ascontiguousarray(np.concatenate([x[1:], x[:1]]))}
    last = _head(moved)[(B - 1) * L:]                        # the same sample in the last slot
    alone = _head({**inp, "B": 1, "x": np.ascontiguousarray(x[:1])})
    assert np.isfinite(first).all()
    assert (_bits(first) == _bits(last)).all(), "the sample's head output depends on its slot in the tile"
    assert (_bits(first) == _bits(alone)).all(), "the sample's head output depends on its neighbours"


@pytest.mark.parametrize("C,L", [(128, 64), (256, 32)])
def test_whole_tile_of_one_sample(C, L):
    inp = _inputs(f"waves_whole_C{C}", C, 1, L)
    r = _ratio(_head(inp), inp)
    print(f"RATIO head waves_whole_C{C} {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("C,B", [(128, 65), (256, 33)])
def test_one_token_samples_give_the_v_projection(C, B):
    inp = _inputs(f"waves_L1_C{C}", C, B, 1)
    W, sub = inp["W"], R.subset(inp)
    x = inp["x"][sub, 0].astype(np.float64)
    mu = x.mean(-1, keepdims=True)
    ln = (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + R.EPS) * W["ln.weight"].astype(np.float64) + W["ln.bias"].astype(np.float64)
    v = ln @ W[IN_W][2 * C:].astype(np.float64).T + W[IN_B][2 * C:].astype(np.float64)
    ref = R.ref64("head", inp)["out"][:, 0]
    assert np.abs(ref - v).max() <= 1e-12 * np.abs(v).max()      # (the reference's softmax of one key is 1 as well)
    got = _head(inp)
    assert np.isfinite(got).all()
    bd = R.bound("head", inp)["out"][:, 0]
    r = float((np.abs(got[sub].astype(np.float64) - v) / bd).max())
    print(f"RATIO head waves_L1_C{C} {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("C,B", [(128, 5), (256, 3)])
def test_ragged_tile_guard(C, B):
    inp = _inputs(f"waves_iso_C{C}", C, B, 16)
    TM, M = 8192 // C, B * 16
    assert M % TM != 0
    got = _head(inp, extra_rows=TM)
    assert np.isnan(got[M:]).all(), "a row beyond M was written"
    assert np.isfinite(got[:M]).all()


def test_two_launches_equal_bits():
    for C, B in ((128, 5), (256, 3)):
        inp = _inputs(f"waves_iso_C{C}", C, B, 16)
        assert (_bits(_head(inp)) == _bits(_head(inp))).all()


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import test_gpu_sa_head_waves as T
out = {}
for C, B, kw in T.AB_CASES:
    inp = T._inputs(f"waves_ab_C{C}_{kw.get('aff')}", C, B, 16, **kw)
    out[f"C{C}_{kw.get('aff')}"] = T._head(inp)
np.savez(sys.argv[2], **out)
"""
AB_CASES = [(128, 5, {}), (256, 3, {}), (128, 5, dict(aff="film", t_count=5)), (256, 3, dict(aff="ab"))]


def test_old_body_against_new(tmp_path):
    procs = {}
    for knob in (0, 3):
        env = {k: v for k, v in os.environ.items() if k != KNOB}
        env[KNOB] = str(knob)
        out = tmp_path / f"knob{knob}.npz"
        procs[knob] = (subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, str(out)], env=env, stdout=subprocess.PIPE,
                                        stderr=subprocess.PIPE, text=True), out)
    got = {}
    for knob, (p, out) in procs.items():
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, (knob, err[-3000:])
        got[knob] = np.load(out)
    for C, B, kw in AB_CASES:
        key = f"C{C}_{kw.get('aff')}"
        inp = _inputs(f"waves_ab_{key}", C, B, 16, **kw)
        r0, r3 = _ratio(got[0][key], inp), _ratio(got[3][key], inp)
        diff = float(np.abs(got[0][key].astype(np.float64) - got[3][key]).max())
        print(f"RATIO head waves_ab_{key} serial {r0:.4f} per-wave {r3:.4f}  max |serial - per-wave| = {diff:.3e}")
        assert r0 <= 1.0 and r3 <= 1.0, (key, r0, r3)
