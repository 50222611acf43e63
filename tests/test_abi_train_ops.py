"""C ABI of the training-launch test hook (include/spdm.h: spdm_op_train) and its argument checks, without a GPU: every call
below is refused before the device is touched (the device pointers are fakes that are never dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_ops_ref as R
from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
INVALID = _lib.SPDM_ERR_INVALID
# dims that must be positive, per op (the others are flags, pads or a count that may be zero)
POSITIVE = {"wgrad": (0, 1, 2, 3, 4, 5, 7, 8), "wgrad_mapped": range(8), "colsum": range(3), "gn_stats": (0, 1), "gn_bwd": range(3),
            "film_bwd": range(5), "mse": range(5), "pool_bwd": range(4), "up_bwd": range(5), "mish_bwd": range(4),
            "ln_fwd": range(2), "ln_bwd": range(2), "gelu_bwd": (0,), "attn_fwd_lse": range(4), "attn_bwd": range(4),
            "gn_bwd_mapped": (0, 1, 2, 4), "simple_tail_bwd": range(6), "silu_bwd": range(3)}


@pytest.fixture(scope="module")
def lib():
    from state_policy_diffusionmodel_amd import build
    build.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_and_library_exports_the_symbol(lib):
    m = re.search(r"\bspdm_op_train\s*\(([^)]*)\)\s*;", _header())
    assert m and re.sub(r"\s+", " ", m.group(1).strip()) == "spdm_op_train_args* args"
    assert "spdm_op_train" in _lib.SYMBOLS and lib.spdm_op_train is not None
    assert lib.spdm_abi_version() == 2                                       # additions only
    assert re.search(r"#define\s+SPDM_ABI_VERSION\s+2\b", open(HDR).read())
    enum = re.search(r"enum\s*\{\s*(SPDM_OPT_WGRAD\b[^}]*)\}", _header()).group(1)
    names = [n.strip().split("=")[0].strip() for n in enum.split(",") if n.strip()]
    assert names == ["SPDM_OPT_" + n.upper() for n in _lib.OP_TRAIN_OPS] + ["SPDM_OPT_COUNT"]
    assert _lib.OP_TRAIN_OPS == R.OPS


def test_struct_matches_the_header():
    hdr = _header()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(SPDM_OP_TRAIN_\w+)\s+(\d+)", hdr)}
    assert consts == {"SPDM_OP_TRAIN_DIMS": _lib.OP_TRAIN_DIMS, "SPDM_OP_TRAIN_BUFS": _lib.OP_TRAIN_BUFS,
                      "SPDM_OP_TRAIN_IDX": _lib.OP_TRAIN_IDX}
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_op_train_args\s*;", hdr).group(1)
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        ctype, var = decl.replace("const ", "").split(None, 1)
        base = ctypes.c_void_p if ("*" in ctype or var.startswith("*")) else c_types[ctype]
        var = var.lstrip("* ")
        m = re.match(r"(\w+)\[(\w+)\]$", var)
        if m:
            n = consts.get(m.group(2)) or int(m.group(2))
            fields.append((m.group(1), base, n))
        else:
            fields.append((var, base, 0))
    A = _lib.SpdmOpTrainArgs
    mine = [(n, getattr(t, "_type_", t), getattr(t, "_length_", 0)) if hasattr(t, "_length_") else (n, t, 0) for n, t in A._fields_]
    assert mine == fields
    assert [f[0] for f in fields] == ["op", "reserved", "dim", "d_buf", "cap", "h_idx", "n_idx", "info"]
    assert ctypes.sizeof(A) == 8 + 80 + 64 + 64 + 16 + 16 + 16                # LP64, no padding
    assert (A.dim.offset, A.d_buf.offset, A.cap.offset, A.h_idx.offset, A.n_idx.offset, A.info.offset) == (8, 88, 152, 216, 232, 248)


class Call:
    """A valid call of one op (the first case of the table) on fake device pointers, to be spoiled one argument at a time."""

    def __init__(self, op, case=None):
        self.op = op
        inp = R.make_inputs(op, case or R.cases(op)[0])
        self.dims, bufs, self.idx, _ = R.launch_plan(op, inp)
        self.bufs = [None if b is None else (4096 * (i + 1), b[1] if b[0] == "out" else int(np.asarray(b[1]).size))
                     for i, b in enumerate(bufs)]

    def run(self, lib):
        a = _lib.SpdmOpTrainArgs()
        a.op = _lib.OP_TRAIN_OPS.index(self.op) if isinstance(self.op, str) else self.op
        for i, v in enumerate(self.dims):
            a.dim[i] = v
        for i, b in enumerate(self.bufs):
            if b is not None:
                a.d_buf[i], a.cap[i] = b
        self.keep = [np.ascontiguousarray(x, np.int32) for x in self.idx]
        for k, x in enumerate(self.keep):
            a.h_idx[k], a.n_idx[k] = (x.ctypes.data if x is not None else None), x.size
        rc = lib.spdm_op_train(ctypes.byref(a))
        assert list(a.info) == [-1] * 4                                      # nothing ran
        return rc, lib.spdm_last_error()


def refused(lib, call, word=None):
    rc, msg = call.run(lib)
    assert rc == INVALID, (call.op, call.dims, rc, msg)
    assert word is None or word.encode() in msg, (word, msg)


def test_null_and_unknown(lib):
    assert lib.spdm_op_train(None) == INVALID
    assert b"null" in lib.spdm_last_error()
    for op in (-1, len(R.OPS), 1000):
        c = Call("gelu_bwd")
        c.op = op
        refused(lib, c, "unknown op")


@pytest.mark.parametrize("op", R.OPS)
def test_every_op_refuses_bad_buffers_and_dimensions(lib, op):
    base = Call(op)
    for i, b in enumerate(base.bufs):
        if b is None:
            continue
        c = Call(op)
        c.bufs[i] = (b[0], b[1] - 1)                                         # one float short
        refused(lib, c, "holds")
        c = Call(op)
        c.bufs[i] = None
        if (op, i) in (("film_bwd", 2), ("film_bwd", 6)):
            refused(lib, c, "go together")
        elif (op, i) not in (("mse", 4), ("ln_bwd", 5)):                      # (optional ones may be left out)
            refused(lib, c, "is null")
    if len(base.bufs) < _lib.OP_TRAIN_BUFS:
        c = Call(op)
        c.bufs.append((4096, 1 << 20))                                       # a buffer the op does not take
        refused(lib, c, "must be null")
    for i in POSITIVE[op]:
        for bad in (0, -1, 2 ** 31):
            c = Call(op)
            c.dims[i] = bad
            refused(lib, c)
    if len(base.dims) < _lib.OP_TRAIN_DIMS:
        c = Call(op)
        c.dims = c.dims + [1]                                                # a dimension the op does not take
        refused(lib, c, "must be 0")
    for k in range(len(base.idx)):
        c = Call(op)
        c.idx[k] = c.idx[k][:-1]                                             # an index array of the wrong length
        refused(lib, c, "entries")
        for bad, where in ((-1, 0), (None, -1)):                             # an index below and beyond its range
            c = Call(op)
            c.idx[k] = c.idx[k].copy()
            lim = {"film_bwd": c.dims[4], "gn_bwd_mapped": c.dims[2]}.get(op, c.dims[4 + k] if op == "wgrad_mapped" else 0)
            c.idx[k][where] = lim if bad is None else bad
            refused(lib, c, "outside")
    if not base.idx:
        c = Call(op)
        c.idx = [np.zeros(1, np.int32)]
        refused(lib, c, "index arrays")


def _spoil(lib, op, word=None, case=None, **dims):
    c = Call(op, case)
    for i, v in dims.items():
        c.dims[int(i[1:])] = v
    for i, b in enumerate(c.bufs):                                           # capacities are no obstacle
        if b is not None:
            c.bufs[i] = (b[0], 2 ** 62)
    refused(lib, c, word)


def test_launcher_limits(lib):
    t9 = R.cases("wgrad")[3]
    assert t9[1]["taps"] == 9
    _spoil(lib, "wgrad", "taps", d3=5)
    _spoil(lib, "wgrad", "W == 1", case=t9, d3=3)                            # 3 taps on a map 8 wide
    _spoil(lib, "wgrad", "Linear", case=t9, d3=1, d6=0)                      # a Linear with a map
    _spoil(lib, "wgrad", "conv9", case=t9, d6=0)
    _spoil(lib, "wgrad", "conv9", d6=1)
    _spoil(lib, "wgrad", "ldy", d7=63)
    _spoil(lib, "wgrad", "ldy", d8=63)
    _spoil(lib, "wgrad", "budget", d4=8192, d5=4096, d7=8192, d8=4096)       # one slab beyond the 16 Mi float budget
    _spoil(lib, "wgrad_mapped", "taps", d3=1)
    _spoil(lib, "wgrad_mapped", "no <= Co", d6=129)
    _spoil(lib, "wgrad_mapped", "ni <= Ci", d7=129)
    _spoil(lib, "colsum", "ld >= C", d2=23)
    _spoil(lib, "gn_stats", "cnt", d2=3 * 4 * 64 + 1)
    for C in (96, 320, 1024):                                                # not a power of two, beyond 512
        _spoil(lib, "gn_bwd", "power of two", d2=C)
        _spoil(lib, "film_bwd", "power of two", d2=C)
    _spoil(lib, "gn_bwd", "gelu", d3=2)
    for C in (32, 96, 576):
        _spoil(lib, "gn_bwd_mapped", "multiple of 64", d2=C)
    _spoil(lib, "gn_bwd_mapped", "nreal", d4=129)
    _spoil(lib, "film_bwd", "t_count", d3=2)
    _spoil(lib, "mse", "lh + H0", d5=2)
    _spoil(lib, "mse", "lw + D", d6=6)
    _spoil(lib, "pool_bwd", "even", d1=3)
    _spoil(lib, "pool_bwd", "even", d2=3)
    _spoil(lib, "up_bwd", "ld >= C", d4=63)
    _spoil(lib, "mish_bwd", "ld >= cond_dim", d2=13)
    _spoil(lib, "silu_bwd", "ld >= cond_dim", d2=13)
    for op in ("ln_fwd", "ln_bwd"):
        for C in (32, 96, 512):
            _spoil(lib, op, "64, 128 or 256", d1=C)
    for op in ("attn_fwd_lse", "attn_bwd"):
        _spoil(lib, op, "not supported", d1=513)                             # L beyond 512
        _spoil(lib, op, "not supported", d2=32)                              # d = 8
        _spoil(lib, op, "not supported", d2=512)                             # d = 128
        _spoil(lib, op, "not supported", d3=3)                               # C % heads
        _spoil(lib, op, "not supported", d1=512)                             # d = 64 at L = 512: beyond the LDS
    _spoil(lib, "simple_tail_bwd", "multiple of 64", d2=96)
    _spoil(lib, "simple_tail_bwd", "multiple of 64", d2=576)
    _spoil(lib, "simple_tail_bwd", "Cr <= Cz", d3=129)
    _spoil(lib, "simple_tail_bwd", "Cr <= Cz", d4=79)
    _spoil(lib, "simple_tail_bwd", "Cr + 32", d3=100)
    _spoil(lib, "simple_tail_bwd", "cemb_ld", d5=31)


def test_index_rules(lib):
    c = Call("film_bwd")
    c.idx[0] = np.array([0, 7, 3], np.int32)                                 # a timestep beyond the table of 7 rows
    refused(lib, c, "outside [0, 7)")
    c = Call("gn_bwd_mapped")
    c.idx[0] = c.idx[0].copy()
    c.idx[0][5] = c.idx[0][4]                                                # a lane named twice
    refused(lib, c, "twice")
    c = Call("gn_bwd_mapped")
    c.idx[0] = c.idx[0].copy()
    c.idx[0][-1] = 128                                                       # beyond the storage width
    refused(lib, c, "outside [0, 128)")
    c = Call("wgrad_mapped")
    c.idx[1] = c.idx[1].copy()
    c.idx[1][0] = 128
    refused(lib, c, "outside [0, 128)")


def test_size_products_beyond_31_and_63_bits(lib):
    big = 2 ** 31 - 2
    _spoil(lib, "gn_stats", "31 bits", d0=2 ** 16, d1=2 ** 15, d2=0)         # B n = 2^31
    _spoil(lib, "gelu_bwd", "outside", d0=2 ** 31)
    _spoil(lib, "pool_bwd", "31 bits", d0=big, d1=big, d2=big, d3=big)       # 2^124: no wrap-around on the way
    _spoil(lib, "up_bwd", "31 bits", d0=big, d1=big, d2=big, d3=big, d4=big)
    _spoil(lib, "colsum", "31 bits", d0=2 ** 20, d1=24, d2=2 ** 12)          # (M - 1) ld + C
    _spoil(lib, "attn_bwd", "31 bits", d0=big)
    _spoil(lib, "ln_bwd", "31 bits", d0=big)
    _spoil(lib, "wgrad", "31 bits", d0=big)                                  # (M - 1) ldy + Co
    _spoil(lib, "mse", "31 bits", d0=big)
    _spoil(lib, "mish_bwd", "31 bits", d0=2 ** 20, d1=2 ** 20)
    _spoil(lib, "simple_tail_bwd", "31 bits", d0=big)
    _spoil(lib, "film_bwd", "31 bits", d0=big, d3=1)
