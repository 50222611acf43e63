"""C ABI of the forward SelfAttention launch test hook (include/spdm.h: spdm_op_sa) and its argument checks, without a GPU: every
call below is refused before the device is touched (the device pointers are fakes that are never dereferenced; the host
weights and timesteps are real, small arrays)."""
import ctypes
import re

import numpy as np
import pytest

import sa_ops_ref as R
from state_policy_diffusionmodel_amd import _lib
from test_abi_stream_ops import _fields, _header, _mine

INVALID = _lib.SPDM_ERR_INVALID
TAKES = {"fused64": ((0, 1, 2, 3), tuple(range(8))), "qkv": ((0,), (0, 1, 2)), "head": ((0,), (0, 1, 2)),
         "tail": ((1, 2, 3), (3, 4, 5, 6, 7)), "core": ((), ())}


@pytest.fixture(scope="module")
def lib():
    from state_policy_diffusionmodel_amd import build
    build.build()
    return _lib.load()


def test_header_declares_and_library_exports_the_symbol(lib):
    m = re.search(r"\bspdm_op_sa\s*\(([^)]*)\)\s*;", _header())
    assert m and re.sub(r"\s+", " ", m.group(1).strip()) == "spdm_op_sa_args* args"
    assert "spdm_op_sa" in _lib.SYMBOLS and lib.spdm_op_sa is not None
    assert lib.spdm_abi_version() == 2                                       # an addition to ABI 2
    enum = re.search(r"enum\s*\{\s*(SPDM_OPA_FUSED64\b[^}]*)\}", _header()).group(1)
    names = [n.strip().split("=")[0].strip() for n in enum.split(",") if n.strip()]
    assert names == ["SPDM_OPA_" + n.upper() for n in _lib.OP_SA_OPS] + ["SPDM_OPA_COUNT"]
    assert _lib.OP_SA_OPS == R.OPS and _lib.OP_SA_KERNELS == R.KERNELS


def test_struct_matches_the_header():
    hdr = _header()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(SPDM_OP_SA_\w+)\s+(\d+)", hdr)}
    assert consts == {"SPDM_OP_SA_DIMS": _lib.OP_SA_DIMS, "SPDM_OP_SA_BUFS": _lib.OP_SA_BUFS,
                      "SPDM_OP_SA_WEIGHTS": _lib.OP_SA_WEIGHTS, "SPDM_OP_SA_VECS": _lib.OP_SA_VECS}
    A = _lib.SpdmOpSaArgs
    assert _mine(A) == _fields(hdr, "spdm_op_sa_args", consts)
    assert ctypes.sizeof(A) == 8 + 80 + 24 + 24 + 32 + 64 + 64 + 16 + 8 + 8 + 56 + 16 + 8 + 16 + 16 + 4 + 20      # LP64, no padding
    assert (A.dim.offset, A.d_buf.offset, A.h_w.offset, A.d_vec.offset, A.d_ab.offset, A.film_on.offset, A.T.offset, A.gn.offset,
            A.d_temb.offset, A.h_t.offset, A.d_outc_w.offset, A.outc_b.offset, A.info.offset) == \
        (8, 88, 136, 168, 296, 312, 320, 328, 384, 400, 424, 440, 444)


class Call:
    """A valid call of one op on fake device pointers, to be spoiled one argument at a time."""

    def __init__(self, op, **spec):
        self.op = op
        C, B, L = spec.get("C", 64), spec.get("B", 3), spec.get("L", 16)
        self.C, self.B, self.L = C, B, L
        crop = spec.get("crop")
        if op == "fused64":
            self.dims = [B, L, 0] + (list((1,) + crop + (spec.get("outc", 0),)) if crop else [0] * 7)
            Q = crop[0] * crop[1] if crop else 0
            self.bufs = [(4096, B * L * 64), None if spec.get("outc") else (8192, B * L * 64), (12288, B * Q) if spec.get("outc") else None]
        elif op == "core":
            self.dims = [B, L, C, spec.get("valu", 0)]
            self.bufs = [(4096, B * L * 3 * C), (8192, B * L * C), None]
        else:
            self.dims = [C, B, L]
            n = B * L * C
            self.bufs = {"qkv": [(4096, n), (8192, 3 * n), None], "head": [(4096, n), (8192, n), None],
                         "tail": [(4096, n), (8192, n), (12288, n)]}[op]
        wi, vi = TAKES[op]
        self.w = {i: np.zeros(((3 if i == 0 else 1) * C, C), np.float32) for i in wi}
        self.vec = {i: (0x10000 * (i + 1), (3 if i == 2 else 1) * C) for i in vi}
        self.ab = (0x200000, B * 2 * C) if spec.get("aff") == "ab" else None
        self.film = None
        if spec.get("aff") == "film":
            tc = spec.get("t_count", 1)
            self.film = dict(t_count=tc, T=5, temb=(0x300000, 5 * C), t=np.arange(tc, dtype=np.int32) % 5, film=(0x400000, B * 2 * C),
                             gn=dict(d_stats=0x500000, stats_cap=B * 4 * 2, slots=4, m_tile=L, n_tiles=2, cnorm=C, d_gamma=0x600000,
                                     d_beta=0x700000, affine_cap=C))
        self.outc = (0x800000, 64, 0.05) if spec.get("outc") else None
        self.extra = {}                                                      # raw fields set last

    def run(self, lib):
        a = _lib.SpdmOpSaArgs()
        a.op = _lib.OP_SA_OPS.index(self.op) if isinstance(self.op, str) else self.op
        for i, v in enumerate(self.dims):
            a.dim[i] = v
        for i, b in enumerate(self.bufs):
            if b is not None:
                a.d_buf[i], a.cap[i] = b
        for i, w in self.w.items():
            a.h_w[i] = w.ctypes.data
        for i, v in self.vec.items():
            a.d_vec[i], a.vec_cap[i] = v
        if self.ab:
            a.d_ab, a.ab_cap = self.ab
        if self.film:
            f = self.film
            a.film_on, a.t_count, a.T = 1, f["t_count"], f["T"]
            if f["temb"]:
                a.d_temb, a.temb_cap = f["temb"]
            if f["t"] is not None:
                a.h_t = f["t"].ctypes.data
            if f["film"]:
                a.d_film, a.film_cap = f["film"]
            for n, v in (f["gn"] or {}).items():
                setattr(a.gn, n, v)
        if self.outc:
            a.d_outc_w, a.outc_w_cap, a.outc_b = self.outc
        for n, v in self.extra.items():
            setattr(a, n, v)
        rc = lib.spdm_op_sa(ctypes.byref(a))
        assert list(a.info) == [-1] * 5                                      # nothing ran
        return rc, lib.spdm_last_error()


def refused(lib, call, word=None):
    rc, msg = call.run(lib)
    assert rc == INVALID, (call.op, call.dims, rc, msg)
    assert msg and (word is None or word.encode() in msg), (word, msg)


VALID = [("fused64", {}), ("fused64", dict(L=128, aff="ab")), ("fused64", dict(L=128, aff="film", t_count=3)),
         ("fused64", dict(L=128, crop=(16, 3, 8, 0, 2), outc=1)), ("qkv", dict(C=128, aff="film")), ("head", dict(C=256, aff="ab")),
         ("tail", dict(C=128, aff="film", t_count=3)), ("core", dict(C=256))]


def test_null_and_unknown_op(lib):
    assert lib.spdm_op_sa(None) == INVALID
    c = Call("core", C=128)
    c.op = 5
    refused(lib, c, "unknown op")
    c.op = -1
    refused(lib, c, "unknown op")


@pytest.mark.parametrize("op,spec", VALID, ids=[f"{o}-{i}" for i, (o, _) in enumerate(VALID)])
def test_every_argument_is_checked(lib, op, spec):
    def spoil(f, word=None):
        c = Call(op, **spec)
        f(c)
        refused(lib, c, word)

    n_dims = {"fused64": 10, "core": 4}.get(op, 3)
    if n_dims < _lib.OP_SA_DIMS:
        spoil(lambda c: c.dims.extend([0] * (n_dims - len(c.dims)) + [1]), "must be 0")
    spoil(lambda c: c.dims.__setitem__(0, -1), "outside")
    spoil(lambda c: c.dims.__setitem__(1, 2 ** 31), "outside")
    iB, iL = (0, 1) if op in ("fused64", "core") else (1, 2)
    spoil(lambda c: c.dims.__setitem__(iB, 0), "positive")
    spoil(lambda c: c.dims.__setitem__(iL, 0), "positive")
    for i in range(_lib.OP_SA_BUFS):
        c0 = Call(op, **spec)
        if c0.bufs[i] is None:
            spoil(lambda c: c.bufs.__setitem__(i, (4096, 1 << 30)), "does not take")
        else:
            spoil(lambda c: c.bufs.__setitem__(i, None), "is null")
            spoil(lambda c: c.bufs.__setitem__(i, (c.bufs[i][0], c.bufs[i][1] - 1)), "holds")
    wi, vi = TAKES[op]
    for i in range(_lib.OP_SA_WEIGHTS):
        if i in wi:
            spoil(lambda c: c.w.pop(i), "needs h_w")
        else:
            spoil(lambda c: c.w.__setitem__(i, np.zeros((4, 4), np.float32)), "does not take h_w")
    for i in range(_lib.OP_SA_VECS):
        if i in vi:
            spoil(lambda c: c.vec.pop(i), "d_vec")
            spoil(lambda c: c.vec.__setitem__(i, (c.vec[i][0], c.vec[i][1] - 1)), "d_vec")
        else:
            spoil(lambda c: c.vec.__setitem__(i, (0x900000, 1024)), "d_vec")
    spoil(lambda c: c.dims.__setitem__(iB, 2 ** 31 - 1), "31 bits")               # B L C beyond 31 bits
    if op == "core":
        spoil(lambda c: setattr(c, "ab", (0x200000, 1 << 20)), "neither")
        spoil(lambda c: c.dims.__setitem__(3, 2), "0 / 1")
        spoil(lambda c: c.dims.__setitem__(2, 96), "C =")
        return
    if op != "fused64":
        spoil(lambda c: c.dims.__setitem__(0, 64), "C =")
    if spec.get("aff") == "ab":
        spoil(lambda c: setattr(c, "ab", (c.ab[0], c.ab[1] - 1)), "ab holds")
        spoil(lambda c: setattr(c, "film", Call(op, **{**spec, "aff": "film"}).film), "mutually exclusive")
    if spec.get("aff") == "film":
        spoil(lambda c: c.film.__setitem__("t_count", 2), "t_count")
        spoil(lambda c: c.film.__setitem__("T", 0), "T must")
        spoil(lambda c: c.film["t"].__setitem__(0, 5), "outside")
        spoil(lambda c: c.film["t"].__setitem__(0, -1), "outside")
        spoil(lambda c: c.film.__setitem__("t", None), "h_t")
        spoil(lambda c: c.film.__setitem__("temb", (c.film["temb"][0], c.film["temb"][1] - 1)), "temb holds")
        spoil(lambda c: c.film.__setitem__("film", (c.film["film"][0], c.film["film"][1] - 1)), "film holds")
        spoil(lambda c: c.film.__setitem__("temb", None), "without temb")
        spoil(lambda c: c.film["gn"].__setitem__("slots", 0), "slots")
        spoil(lambda c: c.film["gn"].__setitem__("slots", 1), "consumer reads")
        spoil(lambda c: c.film["gn"].__setitem__("cnorm", c.C + 1), "cnorm")
        spoil(lambda c: c.film["gn"].__setitem__("d_beta", 0), "gamma and beta")
        spoil(lambda c: c.film["gn"].__setitem__("affine_cap", c.C - 1), "gamma / beta hold")
        spoil(lambda c: c.film["gn"].__setitem__("stats_cap", c.B * 4 * 2 - 1), "statistics hold")
    if op == "fused64" and not spec.get("outc"):
        spoil(lambda c: setattr(c, "outc", (0x800000, 64, 0.0)), "outc")
    if spec.get("outc"):
        spoil(lambda c: setattr(c, "outc", (0x800000, 63, 0.05)), "outc")
        spoil(lambda c: setattr(c, "outc", (0x800000, 64, float("nan"))), "outc")
        spoil(lambda c: setattr(c, "outc", None), "outc")


def test_the_launchers_refusals_come_back_before_the_device(lib):
    """everything the issue's GPU cases expect refused: asked of the launcher itself, dry"""
    bad = [
        ("fused64", dict(L=513), "refuses"),
        ("fused64", dict(L=320, aff="ab"), "refuses"),                               # the two-workgroup form takes no affine
        ("fused64", dict(L=320, aff="film"), "refuses"),
        ("fused64", dict(L=64, crop=(8, 8, 8, 0, 0)), "refuses"),                    # Q = L
        ("fused64", dict(L=256, crop=(27, 5, 8, 0, 0)), "refuses"),                  # Q = 135 above the cap 32 x 4
        ("fused64", dict(L=192, crop=(26, 5, 5, 0, 0), outc=1), "refuses"),
        ("fused64", dict(L=64, crop=(4, 3, 8, 5, 0)), "refuses"),                    # (lh + H0) Wp > L
        ("fused64", dict(L=64, crop=(4, 3, 8, 0, 6)), "refuses"),                    # lw + D > Wp
        ("fused64", dict(L=64, crop=(2, 1, 2 ** 31 - 1, 0, 0)), "exceeds L"),        # (lh + H0) Wp wraps to -2 in 32 bits
        ("fused64", dict(L=64, crop=(3, 1431655766, 2 ** 31 - 1, 0, 0)), "exceeds L"),  # H0 D wraps to 2
        ("fused64", dict(L=64, crop=(2, 1, 8, 2 ** 31 - 1, 0)), "exceeds L"),         # lh + H0 wraps
        ("fused64", dict(L=320, crop=(4, 3, 8, 0, 0)), "refuses"),                   # no crop on two workgroups
        ("qkv", dict(C=128, L=2, aff="film"), "refuses"),                            # sa_tail_film_local: 24 KiB
        ("qkv", dict(C=256, L=2, aff="film"), "refuses"),
        ("tail", dict(C=128, L=2, aff="film"), "refuses"),
        ("tail", dict(C=256, L=2, aff="film"), "refuses"),
        ("head", dict(C=128, L=3), "refuses"),                                       # L does not divide the tile
        ("head", dict(C=256, L=64), "refuses"),
        ("head", dict(C=256, L=1, aff="film"), "refuses"),                           # 33 coefficient rows do not fit
        ("core", dict(C=256, L=320, valu=1), "refuses"),                             # the VALU kernel beyond 160 KiB
        ("core", dict(C=256, L=320), "refuses"),                                     # ... and the MFMA kernel at d = 64
        ("core", dict(C=256, L=512), "refuses"),
    ]
    for op, spec, word in bad:
        refused(lib, Call(op, **spec), word)


def test_film_off_takes_no_film_fields(lib):
    for name, v in (("t_count", 1), ("T", 3), ("d_temb", 0x300000), ("film_cap", 8)):
        c = Call("qkv", C=128)
        c.extra = {name: v}
        refused(lib, c, "film_on 0")
    c = Call("qkv", C=128)
    c.extra = {"film_on": 2}
    refused(lib, c, "film_on is 0 / 1")
