"""C ABI of the encoder / decoder launch test hook (include/spdm.h: spdm_op_frame) and its argument checks, without a GPU: every
call below is refused before the device is touched (the device pointers are fakes that are never dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest

import frame_ops_ref as R
from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
INVALID = _lib.SPDM_ERR_INVALID
# dims that must be positive, per op (the others are a flag, a selector or a count that may be zero)
POSITIVE = {"enc_convs": (0,), "enc_kinks": (0,), "enc_x2": (0,), "enc_dz3": (0,), "enc_dz2": (0,), "enc_conv1_wgrad": (0,),
            "add": (0,), "dec_convs": (0,), "dec_kinks": (0,), "dec_loss": (0,), "dec_bwd6": (0,), "dec_dgrad4": (0,),
            "dec_colsum": (0, 1, 2), "dec_unperm_conv": (0, 1), "dec_unperm_linear": (), "frame_wgrad": (0,)}
FRAME_OPS = [op for op in R.OPS if op.startswith("enc") or op in ("dec_convs", "dec_kinks", "dec_bwd6", "dec_dgrad4")]      # one chunk


@pytest.fixture(scope="module")
def lib():
    from state_policy_diffusionmodel_amd import build
    build.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_and_library_exports_the_symbol(lib):
    m = re.search(r"\bspdm_op_frame\s*\(([^)]*)\)\s*;", _header())
    assert m and re.sub(r"\s+", " ", m.group(1).strip()) == "spdm_op_frame_args* args"
    assert "spdm_op_frame" in _lib.SYMBOLS and lib.spdm_op_frame is not None
    assert lib.spdm_abi_version() == 2                                       # additions only, as for spdm_op_train
    enum = re.search(r"enum\s*\{\s*(SPDM_OPF_ENC_CONVS\b[^}]*)\}", _header()).group(1)
    names = [n.strip().split("=")[0].strip() for n in enum.split(",") if n.strip()]
    assert names == ["SPDM_OPF_" + n.upper() for n in _lib.OP_FRAME_OPS] + ["SPDM_OPF_COUNT"]
    assert _lib.OP_FRAME_OPS == R.OPS


def test_struct_matches_the_header():
    hdr = _header()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(SPDM_OP_FRAME_\w+)\s+(\d+)", hdr)}
    assert consts == {"SPDM_OP_FRAME_DIMS": _lib.OP_FRAME_DIMS, "SPDM_OP_FRAME_BUFS": _lib.OP_FRAME_BUFS}
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_op_frame_args\s*;", hdr).group(1)
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        ctype, var = decl.replace("const ", "").split(None, 1)
        base = ctypes.c_void_p if ("*" in ctype or var.startswith("*")) else c_types[ctype]
        var = var.lstrip("* ")
        m = re.match(r"(\w+)\[(\w+)\]$", var)
        if m:
            fields.append((m.group(1), base, consts.get(m.group(2)) or int(m.group(2))))
        else:
            fields.append((var, base, 0))
    A = _lib.SpdmOpFrameArgs
    mine = [(n, getattr(t, "_type_", t), getattr(t, "_length_", 0)) if hasattr(t, "_length_") else (n, t, 0) for n, t in A._fields_]
    assert mine == fields
    assert [f[0] for f in fields] == ["op", "reserved", "dim", "d_buf", "cap", "d_sq", "sq_cap", "scale", "info", "reserved2"]
    assert ctypes.sizeof(A) == 8 + 32 + 88 + 88 + 16 + 4 + 16 + 4            # LP64, no padding
    assert (A.dim.offset, A.d_buf.offset, A.cap.offset, A.d_sq.offset, A.sq_cap.offset, A.scale.offset, A.info.offset) == \
        (8, 40, 128, 216, 224, 232, 236)


class Call:
    """A valid call of one op (the first case of the table) on fake device pointers, to be spoiled one argument at a time."""

    def __init__(self, op, case=None):
        self.op = op
        inp = R.make_inputs(op, case or R.cases(op)[0])
        self.dims, bufs, _ = R.launch_plan(op, inp)
        self.bufs = [None if b is None else (4096 * (i + 1), b[1] if b[0] == "out" else int(np.asarray(b[1]).size))
                     for i, b in enumerate(bufs)]
        self.sq = (1 << 20, inp["n"]) if op == "dec_loss" or (op == "dec_convs" and inp["train"]) else None
        self.scale = float(inp["scale"]) if op == "dec_bwd6" else 0.0

    def run(self, lib):
        a = _lib.SpdmOpFrameArgs()
        a.op = _lib.OP_FRAME_OPS.index(self.op) if isinstance(self.op, str) else self.op
        for i, v in enumerate(self.dims):
            a.dim[i] = v
        for i, b in enumerate(self.bufs):
            if b is not None:
                a.d_buf[i], a.cap[i] = b
        if self.sq:
            a.d_sq, a.sq_cap = self.sq
        a.scale = self.scale
        rc = lib.spdm_op_frame(ctypes.byref(a))
        assert list(a.info) == [-1] * 4                                      # nothing ran
        return rc, lib.spdm_last_error()


def refused(lib, call, word=None):
    rc, msg = call.run(lib)
    assert rc == INVALID, (call.op, call.dims, rc, msg)
    assert word is None or word.encode() in msg, (word, msg)


def _train_case(op):
    return next(c for c in R.cases(op) if c[1]["train"])


def test_null_and_unknown(lib):
    assert lib.spdm_op_frame(None) == INVALID
    assert b"null" in lib.spdm_last_error()
    for op in (-1, len(R.OPS), 1000):
        c = Call("add")
        c.op = op
        refused(lib, c, "unknown op")


@pytest.mark.parametrize("op", R.OPS)
def test_every_op_refuses_bad_buffers_and_dimensions(lib, op):
    variants = [None] if op not in ("enc_convs", "dec_convs") else [None, _train_case(op)]
    for case in variants:
        base = Call(op, case)
        for i, b in enumerate(base.bufs):
            if b is None:
                c = Call(op, case)
                c.bufs[i] = (4096, 1 << 30)                                  # a buffer that goes with train only
                refused(lib, c, "must be null")
                continue
            c = Call(op, case)
            c.bufs[i] = (b[0], b[1] - 1)                                     # one float short
            refused(lib, c, "holds")
            c = Call(op, case)
            c.bufs[i] = None
            refused(lib, c, "is null")
        if len(base.bufs) < _lib.OP_FRAME_BUFS:
            c = Call(op, case)
            c.bufs.append((4096, 1 << 20))                                   # a buffer the op does not take
            refused(lib, c, "must be null")
        c = Call(op, case)
        if base.sq:
            c.sq = (base.sq[0], base.sq[1] - 1)                              # one double short
            refused(lib, c, "doubles")
            c = Call(op, case)
            c.sq = None
            refused(lib, c, "d_sq is null")
        else:
            c.sq = (1 << 20, 1 << 20)                                        # d_sq where the op does not take it
            refused(lib, c, "must be null")
        if op != "dec_bwd6":
            c = Call(op, case)
            c.scale = 1.0
            refused(lib, c, "scale")
    for i in POSITIVE[op]:
        for bad in (0, -1, 2 ** 31):
            c = Call(op)
            c.dims[i] = bad
            refused(lib, c)
    if len(base.dims) < _lib.OP_FRAME_DIMS:
        c = Call(op)
        c.dims = c.dims + [0] * (_lib.OP_FRAME_DIMS - 1 - len(c.dims)) + [1]  # a dimension the op does not take
        refused(lib, c, "must be 0")


def _spoil(lib, op, word=None, case=None, scale=None, **dims):
    c = Call(op, case)
    for i, v in dims.items():
        c.dims[int(i[1:])] = v
    for i, b in enumerate(c.bufs):                                           # capacities are no obstacle
        if b is not None:
            c.bufs[i] = (b[0], 2 ** 62)
    if c.sq:
        c.sq = (c.sq[0], 2 ** 62)
    if scale is not None:
        c.scale = scale
    refused(lib, c, word)


def test_launcher_limits(lib):
    """what the launchers accept and the two passes cannot produce"""
    for op in FRAME_OPS:
        _spoil(lib, op, "frames", d0=R.CHUNK + 1)                            # more than one chunk of the passes
    _spoil(lib, "enc_convs", "train", d1=2)
    _spoil(lib, "dec_convs", "train", d1=2)
    for bad in (float("nan"), float("inf")):
        _spoil(lib, "dec_bwd6", "finite", scale=bad)
    for C, fold in ((192, 4), (256, 4), (32, 4), (9216, 4), (64, 1), (128, 2), (9216, 2)):    # launch_decoder_colsum takes any C % 64 == 0
        _spoil(lib, "dec_colsum", "(C, fold)", d1=C, d2=fold)
    _spoil(lib, "dec_colsum", "one chunk", d0=R.CHUNK * 576 + 1)
    _spoil(lib, "dec_colsum", "one chunk", d0=R.CHUNK * 144 + 1, d1=128)
    _spoil(lib, "dec_colsum", "one chunk", d0=R.CHUNK + 1, d1=9216, d2=1)
    for cin, cout in ((64, 16), (32, 32), (3, 16), (1, 1), (128, 64)):       # launch_decoder_unperm_conv takes any cin, cout
        _spoil(lib, "dec_unperm_conv", "(cin, cout)", d0=cin, d1=cout)
    _spoil(lib, "frame_wgrad", "which", d1=6)
    for which, rows in enumerate((1, 144, 576, 576, 144, 1)):
        _spoil(lib, "frame_wgrad", "one chunk", d0=R.CHUNK * rows + 1, d1=which)


def test_size_products_beyond_31_bits(lib):
    # the frame limit keeps every per-frame extent below 2^31 (2048 x 36864 = 2^26.2); the free sizes are ADD's n and the M of the
    # column sum and the weight gradient, bounded by a chunk's rows
    _spoil(lib, "add", "outside", d0=2 ** 31)
    _spoil(lib, "dec_colsum", "outside", d0=2 ** 31)
    _spoil(lib, "frame_wgrad", "outside", d0=2 ** 31)
    for op in FRAME_OPS:
        _spoil(lib, op, "outside", d0=2 ** 31)
        _spoil(lib, op, None, d0=2 ** 31 - 1)
    for op, word in (("add", "holds"), ("dec_loss", "doubles")):            # the largest n: the capacities decide
        c = Call(op)
        c.dims[0] = 2 ** 31 - 1
        refused(lib, c, word)
    _spoil(lib, "dec_loss", "outside", d0=2 ** 31)
