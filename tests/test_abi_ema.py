"""C ABI of the EMA step (include/spdm.h: spdm_ema_segment, spdm_ema_step) and its refusals, without a GPU: every refusal
comes back before the device is touched, with the project's code and a message, and leaves the arrays it was given alone."""
import ctypes
import os
import re

import numpy as np

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")


def test_header_struct_and_binding_agree():
    hdr = open(HDR).read()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_ema_segment\s*;", hdr)
    assert m
    fields = [f.split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()]
    assert fields == [f[0] for f in _lib.SpdmEmaSegment._fields_] == ["d_ema", "d_param", "numel"]
    assert ctypes.sizeof(_lib.SpdmEmaSegment) == 24
    decl = re.search(r"\bspdm_ema_step\s*\(([^)]*)\)\s*;", hdr)
    assert decl and len(decl.group(1).split(",")) == len(_lib.SYMBOLS["spdm_ema_step"][1]) == 5
    assert "const spdm_ema_segment* h_segments" in decl.group(1) and "float one_minus_decay" in decl.group(1)


def test_symbol_is_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.spdm_ema_step is not None and lib.spdm_ema_step.restype is ctypes.c_int32
    assert re.search(r"#define\s+SPDM_ABI_VERSION\s+2\b", open(HDR).read()) and lib.spdm_abi_version() == 2


def _aligned(n, fill):
    """n float32 at a 16-byte aligned host address (never dereferenced by a refused call), inside a guard of other values"""
    raw = np.full(n + 16, -7.0, dtype=np.float32)
    off = ((-raw.ctypes.data) % 16) // 4
    view = raw[off:off + n]
    assert view.ctypes.data % 16 == 0
    view[:] = fill
    return raw, view


class _Arrays:
    def __init__(self):
        self.raw_e, self.ema = _aligned(32, 1.5)
        self.raw_p, self.p = _aligned(32, 2.5)
        self.before = (self.raw_e.copy(), self.raw_p.copy())

    def untouched(self):
        return np.array_equal(self.raw_e, self.before[0]) and np.array_equal(self.raw_p, self.before[1])


def _call(segs, n=None, omd=0.1):
    lib = _lib.load()
    arr = (_lib.SpdmEmaSegment * max(1, len(segs)))(*segs) if segs is not None else None
    return lib.spdm_ema_step(0, arr, len(segs) if n is None else n, omd, ctypes.c_void_p())


def test_every_refusal_without_a_gpu():
    INVALID = _lib.SPDM_ERR_INVALID
    lib = _lib.load()
    a = _Arrays()
    e, p, S = a.ema.ctypes.data, a.p.ctypes.data, _lib.SpdmEmaSegment
    good = S(e, p, 32)
    cases = {
        "null table": lambda: _call(None, n=1),
        "no segments": lambda: _call([good], n=0),
        "negative count": lambda: _call([good], n=-1),
        "five segments": lambda: _call([good] * 5),
        "null ema": lambda: _call([S(None, p, 32)]),
        "null param": lambda: _call([S(e, None, 32)]),
        "null in a later segment": lambda: _call([good, S(e, None, 32)]),
        "empty": lambda: _call([S(e, p, 0)]),
        "empty later": lambda: _call([good, S(e, p, 0)]),
        "ema misaligned": lambda: _call([S(e + 4, p, 16)]),
        "param misaligned": lambda: _call([S(e, p + 8, 16)]),
        "misaligned later": lambda: _call([good, S(e, p + 4, 16)]),
        "same array": lambda: _call([S(e, e, 32)]),
        "param inside ema": lambda: _call([S(e, e + 16, 16)]),
        "ema inside param": lambda: _call([S(p + 64, p, 32)]),
        "last float shared": lambda: _call([S(e, e + 16 * 4 - 16, 13)]),
        "omd nan": lambda: _call([good], omd=float("nan")),
        "omd above 1": lambda: _call([good], omd=1.0000001),
        "omd negative": lambda: _call([good], omd=-1e-9),
        "omd inf": lambda: _call([good], omd=float("inf")),
    }
    for name, call in cases.items():
        assert call() == INVALID, name
        msg = lib.spdm_last_error()
        assert msg and b"ema_step" in msg, (name, msg)
        assert a.untouched(), name
    assert b"one_minus_decay" in lib.spdm_last_error()
