"""C ABI of the forward streaming-launch test hook (include/spdm.h: spdm_op_stream) and its argument checks, without a GPU: every
call below is refused before the device is touched (the device pointers are fakes that are never dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest

import stream_ops_ref as R
from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
INVALID = _lib.SPDM_ERR_INVALID
# dims that must be positive, per op (the others are offsets, flags, counts that may be zero, or adv)
POSITIVE = {"conv_in": range(5), "pool": range(4), "upcat": range(4), "film_apply": range(5), "film_coef": range(5),
            "layernorm": range(2), "mish_pad": range(3), "silu_pad": range(3), "silu": (0,), "dc_finish": range(3),
            "simple_tail": range(9), "splitk_combine": range(4), "out_step": (0, 1, 2, 3, 4, 10)}
FIRST_WITH = lambda op, pred: next(c for c in R.cases(op) if pred(c[1]))


@pytest.fixture(scope="module")
def lib():
    from state_policy_diffusionmodel_amd import build
    build.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_and_library_exports_the_symbol(lib):
    m = re.search(r"\bspdm_op_stream\s*\(([^)]*)\)\s*;", _header())
    assert m and re.sub(r"\s+", " ", m.group(1).strip()) == "spdm_op_stream_args* args"
    assert "spdm_op_stream" in _lib.SYMBOLS and lib.spdm_op_stream is not None
    assert lib.spdm_abi_version() == 2                                       # additions only, as for spdm_op_train
    enum = re.search(r"enum\s*\{\s*(SPDM_OPS_CONV_IN\b[^}]*)\}", _header()).group(1)
    names = [n.strip().split("=")[0].strip() for n in enum.split(",") if n.strip()]
    assert names == ["SPDM_OPS_" + n.upper() for n in _lib.OP_STREAM_OPS] + ["SPDM_OPS_COUNT"]
    assert _lib.OP_STREAM_OPS == R.OPS


def _fields(hdr, name, consts):
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", hdr).group(1)
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
               "spdm_op_stream_gn": _lib.SpdmOpStreamGn}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        ctype, var = decl.replace("const ", "").split(None, 1)
        base = ctypes.c_void_p if ("*" in ctype or var.startswith("*")) else c_types[ctype]
        var = var.lstrip("* ")
        m = re.match(r"(\w+)\[(\w+)\]$", var)
        fields.append((m.group(1), base, consts.get(m.group(2)) or int(m.group(2))) if m else (var, base, 0))
    return fields


def _mine(A):
    return [(n, getattr(t, "_type_", t), getattr(t, "_length_", 0)) if hasattr(t, "_length_") else (n, t, 0) for n, t in A._fields_]


def test_structs_match_the_header():
    hdr = _header()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(SPDM_OP_STREAM_\w+)\s+(\d+)", hdr)}
    assert consts == {"SPDM_OP_STREAM_DIMS": _lib.OP_STREAM_DIMS, "SPDM_OP_STREAM_BUFS": _lib.OP_STREAM_BUFS,
                      "SPDM_OP_STREAM_IDX": _lib.OP_STREAM_IDX, "SPDM_OP_STREAM_GN": _lib.OP_STREAM_GN}
    G, A = _lib.SpdmOpStreamGn, _lib.SpdmOpStreamArgs
    assert _mine(G) == _fields(hdr, "spdm_op_stream_gn", consts)
    assert _mine(A) == _fields(hdr, "spdm_op_stream_args", consts)
    assert ctypes.sizeof(G) == 8 + 8 + 16 + 8 + 8 + 8                          # LP64, no padding
    assert (G.stats_cap.offset, G.slots.offset, G.cnorm.offset, G.d_gamma.offset, G.affine_cap.offset) == (8, 16, 28, 32, 48)
    assert ctypes.sizeof(A) == 8 + 112 + 64 + 64 + 8 + 8 + 112 + 8 + 8 + 8 + 8 + 8 + 4 + 16 + 4
    assert (A.dim.offset, A.d_buf.offset, A.cap.offset, A.h_idx.offset, A.n_idx.offset, A.gn.offset, A.d_stats_out.offset,
            A.d_words.offset, A.seed.offset, A.bias.offset, A.info.offset) == (8, 120, 184, 248, 256, 264, 376, 392, 400, 416, 420)


class Call:
    """A valid call of one op (the first case of the table, or the given one) on fake device pointers, to be spoiled one argument
    at a time."""

    def __init__(self, op, case=None):
        self.op = op
        P = R.launch_plan(op, R.make_inputs(op, case or R.cases(op)[0]))
        self.dims, self.idx = list(P["dims"]), P["idx"]
        self.bufs = [None if b is None else (4096 * (i + 1), b[1] if b[0] == "out" else int(np.asarray(b[1]).size))
                     for i, b in enumerate(P["bufs"])]
        self.gn = [None if g is None else dict(d_stats=0x100000 * (k + 1), stats_cap=g["stats"].size, slots=g["slots"], m_tile=g["m_tile"],
                                               n_tiles=g["n_tiles"], cnorm=g["cnorm"], d_gamma=0x200000, d_beta=0x300000,
                                               affine_cap=len(g["gamma"])) for k, g in enumerate(P["gn"])]
        self.stats_out = None if P["stats_out"] is None else (0x400000, P["stats_out"])
        self.words = 0x500000 if P["words"] else None

    def run(self, lib):
        a = _lib.SpdmOpStreamArgs()
        a.op = _lib.OP_STREAM_OPS.index(self.op) if isinstance(self.op, str) else self.op
        for i, v in enumerate(self.dims):
            a.dim[i] = v
        for i, b in enumerate(self.bufs):
            if b is not None:
                a.d_buf[i], a.cap[i] = b
        if self.idx is not None:
            self.keep = np.ascontiguousarray(self.idx, np.int32)
            a.h_idx[0], a.n_idx[0] = self.keep.ctypes.data, self.keep.size
        for k, g in enumerate(self.gn):
            for n, v in (g or {}).items():
                setattr(a.gn[k], n, v)
        if self.stats_out is not None:
            a.d_stats_out, a.stats_out_cap = self.stats_out
        a.d_words = self.words
        rc = lib.spdm_op_stream(ctypes.byref(a))
        assert list(a.info) == [-1] * 4                                      # nothing ran
        return rc, lib.spdm_last_error()


def refused(lib, call, word=None):
    rc, msg = call.run(lib)
    assert rc == INVALID, (call.op, call.dims, rc, msg)
    assert msg and (word is None or word.encode() in msg), (word, msg)


def test_null_and_unknown(lib):
    assert lib.spdm_op_stream(None) == INVALID
    assert b"null" in lib.spdm_last_error()
    for op in (-1, len(R.OPS), 1000):
        c = Call("silu")
        c.op = op
        refused(lib, c, "unknown op")


OPTIONAL = {("film_apply", 1), ("film_apply", 2), ("film_coef", 0), ("film_coef", 1), ("dc_finish", 1), ("out_step", 5), ("out_step", 7)}


def _full_case(op):
    """a case of the op that uses every buffer, index array and statistics input it can"""
    if op in ("film_apply", "film_coef"):
        return FIRST_WITH(op, lambda k: k["temb"] and k["film"] and k["gn"] and (op == "film_coef" or k["row_stats"]))
    if op == "dc_finish":
        return FIRST_WITH(op, lambda k: k["res"] and k["gn"])
    if op == "upcat":
        return FIRST_WITH(op, lambda k: k["Cs"] and k["gn"] and k["gn_skip"])
    if op in ("pool", "simple_tail"):
        return FIRST_WITH(op, lambda k: k["gn"])
    if op == "conv_in":
        return FIRST_WITH(op, lambda k: k["adv"] == -1)
    if op == "out_step":
        return FIRST_WITH(op, lambda k: k["mode"] == 2 and k["noise"] == "buffer" and k["inp_h"] and k["history"])
    return R.cases(op)[0]


@pytest.mark.parametrize("op", R.OPS)
def test_every_op_refuses_bad_buffers_and_dimensions(lib, op):
    case = _full_case(op)
    base = Call(op, case)                                                    # (itself valid: it would reach the device, and is not run)
    for i, b in enumerate(base.bufs):
        if b is None:
            continue
        c = Call(op, case)
        c.bufs[i] = (b[0], b[1] - 1)                                         # one float short
        refused(lib, c, "holds")
        c = Call(op, case)
        c.bufs[i] = None
        if (op, i) in (("film_apply", 1), ("film_coef", 0)):                 # temb left out: its timesteps have no table
            refused(lib, c)
        elif (op, i) not in OPTIONAL:
            refused(lib, c, "is null")
    if len(base.bufs) < _lib.OP_STREAM_BUFS:
        c = Call(op, case)
        c.bufs.append((4096, 1 << 20))                                       # a buffer the op does not take
        refused(lib, c, "must be null")
    for i in POSITIVE[op]:
        for bad in (0, -1, 2 ** 31):
            c = Call(op, case)
            c.dims[i] = bad
            refused(lib, c)
    if len(base.dims) < _lib.OP_STREAM_DIMS:
        c = Call(op, case)
        c.dims = c.dims + [1]                                                # a dimension the op does not take
        refused(lib, c, "must be 0")
    if base.idx is not None:
        c = Call(op, case)
        c.idx = c.idx[:-1]                                                   # an index array of the wrong length
        refused(lib, c, "entries")
        c = Call(op, case)
        c.idx = None
        refused(lib, c, "entries")
        for bad in (-1, None):                                               # a timestep below and beyond its range
            if bad is None and op == "conv_in":
                continue                                                     # (conv_in stores its timesteps, it does not index with them)
            c = Call(op, case)
            c.idx = c.idx.copy()
            c.idx[-1] = c.dims[8 if op == "simple_tail" else 4] if bad is None else bad    # T: one beyond the table
            refused(lib, c, "outside")
    else:
        c = Call(op, case)
        c.idx = np.zeros(1, np.int32)
        refused(lib, c, "index arrays")
    # statistics out and the words
    if base.stats_out is None:
        c = Call(op, case)
        c.stats_out = (0x400000, 1 << 20)
        refused(lib, c, "d_stats_out")
    else:
        c = Call(op, case)
        c.stats_out = (base.stats_out[0], base.stats_out[1] - 1)
        refused(lib, c, "doubles")
        if op != "film_apply":
            c = Call(op, case)
            c.stats_out = None
            refused(lib, c, "d_stats_out is null")
    c = Call(op, case)
    c.words = None if base.words else 0x500000
    refused(lib, c, "d_words")
    # a pending GroupNorm
    for k, g in enumerate(base.gn):
        if g is None:
            c = Call(op, case)
            c.gn[k] = dict(d_stats=0x100000, stats_cap=1 << 20, slots=64, m_tile=1, n_tiles=1, cnorm=4, d_gamma=0x200000, d_beta=0x300000,
                           affine_cap=1 << 20)
            if op not in R.GN_CONSUMERS or (op != "upcat" and k == 1):
                refused(lib, c, "no pending GroupNorm")
            continue
        for field, bad, word in (("stats_cap", g["stats_cap"] - 1, "doubles"), ("slots", g["slots"] - 2, "consumer reads"), ("slots", 0, ">= 1"),
                                 ("m_tile", 0, ">= 1"), ("n_tiles", -1, ">= 1"), ("cnorm", 0, "cnorm"), ("cnorm", 2048, "cnorm"),
                                 ("d_gamma", None, "gamma and beta"), ("d_beta", None, "gamma and beta"),
                                 ("affine_cap", g["affine_cap"] - 1, "gamma / beta hold")):
            c = Call(op, case)
            c.gn[k] = dict(g, **{field: bad})
            refused(lib, c, word)
        c = Call(op, case)
        c.gn[k] = dict(g, d_stats=None)                                      # the geometry of statistics that are not there
        refused(lib, c, "must be empty")


def _spoil(lib, op, word=None, case=None, **dims):
    c = Call(op, case)
    for i, v in dims.items():
        c.dims[int(i[1:])] = v
    for i, b in enumerate(c.bufs):                                           # capacities are no obstacle
        if b is not None:
            c.bufs[i] = (b[0], 2 ** 62)
    for g in c.gn:
        if g is not None:
            g.update(stats_cap=2 ** 62, affine_cap=2 ** 62, slots=2 ** 20)
    if c.stats_out is not None:
        c.stats_out = (c.stats_out[0], 2 ** 62)
    refused(lib, c, word)


def test_launcher_limits_and_what_the_launchers_do_not_check(lib):
    _spoil(lib, "conv_in", "lh + H0", d5=1)
    _spoil(lib, "conv_in", "lw + D", d6=8)
    _spoil(lib, "conv_in", "LDS", d1=64, d3=2048, d4=8)                      # 16392 floats of image
    adv = FIRST_WITH("conv_in", lambda k: k["adv"] == -1)
    _spoil(lib, "conv_in", "step0 < n_steps", case=adv, d10=5)
    _spoil(lib, "conv_in", "adv <= n_steps", case=adv, d8=6)
    _spoil(lib, "conv_in", "outside", case=adv, d8=-3)
    _spoil(lib, "conv_in", "adv -2", d9=3)                                   # no bookkeeping, yet a step count
    _spoil(lib, "pool", "even", d1=3)
    _spoil(lib, "pool", "even", d2=5)
    for C in (6, 1028):
        _spoil(lib, "pool", "multiple of 4", d3=C)
        _spoil(lib, "dc_finish", "multiple of 4", d2=C)
    _spoil(lib, "upcat", "multiples of 4", d3=66)
    _spoil(lib, "upcat", "multiples of 4", d4=2)
    _spoil(lib, "upcat", "<= 1024", d3=1024, d4=64)
    noskip = FIRST_WITH("upcat", lambda k: k["Cs"] == 0)
    c = Call("upcat", noskip)
    c.bufs[1] = (4096, 1 << 30)                                              # a skip tensor of no channels
    refused(lib, c, "must be null")
    for C in (0, 6, 48, 192, 2048):                                          # launch_film_apply would divide by C / 4 == 0
        _spoil(lib, "film_apply", None if C == 0 else "divide 256", d2=C)
    _spoil(lib, "film_apply", "t_count", d3=2, case=FIRST_WITH("film_apply", lambda k: k["B"] == 3))
    rs = FIRST_WITH("film_apply", lambda k: k["row_stats"])
    _spoil(lib, "film_apply", "row statistics", case=rs, d2=512)
    _spoil(lib, "film_coef", "t_count", d3=2, case=FIRST_WITH("film_coef", lambda k: k["B"] == 3))
    _spoil(lib, "film_apply", "without temb", case=FIRST_WITH("film_apply", lambda k: not k["temb"]), d4=3)
    for C in (32, 96, 1024):
        _spoil(lib, "layernorm", "64, 128, 256 or 512", d1=C)
    for op in ("mish_pad", "silu_pad"):                                      # launch_mish_pad checks nothing
        _spoil(lib, op, "Kp >= cond_dim", d2=29)
    st = FIRST_WITH("simple_tail", lambda k: (k["Co"], k["Cr"], k["B"]) == (128, 96, 3))
    assert (st[1]["Co"], st[1]["Cr"], st[1]["src_C"]) == (128, 96, 128)
    _spoil(lib, "simple_tail", "multiples of 4", case=st, d3=94)
    _spoil(lib, "simple_tail", "Cr + 32 <= Co", case=st, d3=100, d5=100)
    _spoil(lib, "simple_tail", "Cr <= src_C", case=st, d4=64)
    _spoil(lib, "simple_tail", "temb_ld >= Cr", case=st, d5=92)
    _spoil(lib, "simple_tail", "cemb_ld >= 32", case=st, d6=28)
    _spoil(lib, "simple_tail", "Co <= 1024", case=st, d2=1028)
    _spoil(lib, "simple_tail", "t_count", case=st, d7=2 if st[1]["B"] != 2 else 3)   # launch_simple_tail takes any t_count >= 1
    _spoil(lib, "splitk_combine", "ksplit >= 2", d3=1)
    _spoil(lib, "splitk_combine", "multiple of 4", d2=66)
    os_ = _full_case("out_step")
    _spoil(lib, "out_step", "lh + H0", case=os_, d5=3)                       # launch_out_step checks none of these
    _spoil(lib, "out_step", "lw + D", case=os_, d6=9)
    _spoil(lib, "out_step", "outside [0, 5)", case=os_, d9=5)
    _spoil(lib, "out_step", "inp_h", case=os_, d11=os_[1]["H0"] + 1)
    for d in ("d7", "d12", "d13"):
        _spoil(lib, "out_step", "0 / 1", case=os_, **{d: 2})
    _spoil(lib, "out_step", "mode 0, 1 or 2", case=os_, d8=3)
    c = Call("out_step", os_)
    c.dims[8] = 1                                                            # from the features: eps is not an input
    c.bufs[0], c.bufs[1] = (4096, 2 ** 40), (8192, 64)
    refused(lib, c, "must be null")
    c = Call("out_step", os_)
    c.dims[11] = 0                                                           # in-painting rows without a height
    refused(lib, c, "must be null")


def test_slot_counts_follow_the_consumers_reads(lib):
    """B = 3, HW = 24, m_tile = 13: samples touch 2, 3 and 2 row tiles; with n_tiles = 5 the consumer reads up to 15 slots"""
    case = FIRST_WITH("pool", lambda k: k["gn"] == "straddle" and k["H"] * k["W"] == 24 and k["B"] == 3)
    g = Call("pool", case).gn[0]
    assert (g["m_tile"], g["n_tiles"]) == (13, 5) and g["slots"] == 16
    for slots, word in ((15, "doubles"), (14, "consumer reads"), (10, "consumer reads")):
        c = Call("pool", case)
        c.gn[0] = dict(g, slots=slots, stats_cap=3 * slots * 2 - 1)          # 15 slots pass the count and fail on the capacity only
        refused(lib, c, word)


def test_size_products_beyond_31_bits(lib):
    big = 2 ** 31 - 2
    _spoil(lib, "silu", "outside", d0=2 ** 31)
    _spoil(lib, "pool", "31 bits", d0=big, d1=big, d2=big, d3=64)
    _spoil(lib, "upcat", "31 bits", d0=big)
    _spoil(lib, "film_apply", "31 bits", d0=big, d3=1)
    _spoil(lib, "film_coef", "31 bits", d0=2 ** 23, d3=1, d2=256)            # B 2C = 2^32
    _spoil(lib, "layernorm", "31 bits", d0=2 ** 25)
    _spoil(lib, "mish_pad", "31 bits", d0=2 ** 20, d2=2 ** 12)
    _spoil(lib, "dc_finish", "31 bits", d0=big)
    _spoil(lib, "simple_tail", "31 bits", d1=big)
    _spoil(lib, "splitk_combine", "31 bits", d0=2 ** 12, d1=2 ** 10, d2=256, d3=9)   # the slabs together
    _spoil(lib, "conv_in", "31 bits", d0=big)
    _spoil(lib, "out_step", "31 bits", d0=big, case=_full_case("out_step"))
