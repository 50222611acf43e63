"""C ABI of the validation-loss entry points (include/spdm.h: spdm_loss_terms, spdm_unet_forward_dt) and their argument checks,
without a GPU: every call below is refused before the device is touched."""
import ctypes
import os
import re

import pytest

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
FIELDS = ["B", "H", "D", "reserved", "d_eps", "d_noise", "slot_offset", "n_slots", "d_terms", "d_t_in", "d_slot_t"]
INVALID = _lib.SPDM_ERR_INVALID


@pytest.fixture(scope="module")
def lib():
    from state_policy_diffusionmodel_amd import build
    build.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def _struct_fields(name):
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", _header())
    assert m, name
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
    fields = []
    for decl in (d.strip() for d in m.group(1).split(";")):
        if not decl:
            continue
        ctype, var = decl.replace("const ", "").split(None, 1)
        if "*" in ctype or var.startswith("*"):
            fields.append((var.lstrip("* "), ctypes.c_void_p))
        else:
            fields.append((var, c_types[ctype]))
    return fields


def test_header_declares_and_library_exports_the_symbols(lib):
    fwd = "spdm_handle* h, int32_t B, const float* d_x, const int32_t* %s, int32_t t_count, const float* d_cond, float* d_eps, void* stream"
    want = {"spdm_loss_terms": "int32_t device, const spdm_loss_terms_args* a, void* stream",
            "spdm_unet_forward_dt": fwd % "d_t",
            "spdm_unet_forward": fwd % "h_t"}                                # the two forwards differ in where t lives only
    for name, sig in want.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", _header())
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1).strip()) == sig
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert _lib.SYMBOLS["spdm_unet_forward_dt"] == _lib.SYMBOLS["spdm_unet_forward"]
    assert lib.spdm_abi_version() == 2                                       # additions only


def test_struct_matches_the_header():
    fields = _struct_fields("spdm_loss_terms_args")
    assert [f[0] for f in fields] == FIELDS
    assert list(_lib.SpdmLossTermsArgs._fields_) == fields
    A = _lib.SpdmLossTermsArgs
    assert ctypes.sizeof(A) == 72                                            # 4 x 4, 2 x 8, 2 x 8, 3 x 8 (LP64), no padding
    assert A.d_eps.offset == 16 and A.slot_offset.offset == 32 and A.n_slots.offset == 40 and A.d_terms.offset == 48
    assert A.d_slot_t.offset == 64


def _terms(lib, **kw):
    # 5 samples of 31 x 5 into slots 3 .. 7 of 8.  Device pointers that are never dereferenced.
    base = dict(B=5, H=31, D=5, reserved=0, d_eps=4096, d_noise=8192, slot_offset=3, n_slots=8, d_terms=12288, d_t_in=16384,
                d_slot_t=20480)
    base.update(kw)
    return lib.spdm_loss_terms(0, ctypes.byref(_lib.SpdmLossTermsArgs(**base)), ctypes.c_void_p())


def test_loss_terms_refuses_invalid_arguments_without_a_gpu(lib):
    assert lib.spdm_loss_terms(0, None, ctypes.c_void_p()) == INVALID
    assert b"null" in lib.spdm_last_error()
    for name in ("d_eps", "d_noise", "d_terms"):
        assert _terms(lib, **{name: None}) == INVALID, name
        assert b"null" in lib.spdm_last_error()
    for name in ("B", "H", "D"):
        for bad in (0, -1):
            assert _terms(lib, **{name: bad}) == INVALID, (name, bad)
    assert _terms(lib, slot_offset=-1) == INVALID
    assert b"negative" in lib.spdm_last_error()
    assert _terms(lib, slot_offset=4) == INVALID                             # 4 + 5 > 8
    assert b"n_slots" in lib.spdm_last_error()
    assert _terms(lib, n_slots=7) == INVALID
    assert _terms(lib, B=9, slot_offset=0) == INVALID                        # more samples than slots
    assert _terms(lib, slot_offset=2 ** 63 - 3, n_slots=2 ** 63 - 1) == INVALID     # no overflow in slot_offset + B
    assert _terms(lib, n_slots=0, slot_offset=0) == INVALID
    assert _terms(lib, d_t_in=None) == INVALID                               # exactly one of the pair
    assert b"go together" in lib.spdm_last_error()
    assert _terms(lib, d_slot_t=None) == INVALID
    assert _terms(lib, H=2 ** 16, D=2 ** 15) == INVALID                      # H x D beyond 31 bits
    assert b"loss_terms" in lib.spdm_last_error()


def test_unet_forward_dt_refuses_a_null_handle_without_a_gpu(lib):
    p = ctypes.c_void_p
    assert lib.spdm_unet_forward_dt(None, 1, p(4096), p(8192), 1, None, p(12288), p()) == INVALID
    assert lib.spdm_unet_forward(None, 1, p(4096), p(8192), 1, None, p(12288), p()) == INVALID
