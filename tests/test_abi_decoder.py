"""C ABI of the decoder's entry points (include/spdm.h), without a GPU."""
import ctypes
import os
import re

from state_policy_diffusionmodel_amd import _lib

NEW = ("spdm_decoder_create", "spdm_decoder_forward", "spdm_decoder_train_loss", "spdm_decoder_backward",
       "spdm_decoder_update_weights", "spdm_decoder_destroy")


def test_header_declares_and_library_exports_the_six_symbols():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    assert re.search(r"typedef\s+struct\s+spdm_decoder\s+spdm_decoder\s*;", hdr)


def test_abi_version_is_still_2():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")).read()
    assert re.search(r"#define\s+SPDM_ABI_VERSION\s+2\b", hdr)
    assert _lib.ABI_VERSION == 2 and _lib.load().spdm_abi_version() == 2


def test_null_arguments_are_invalid_without_a_gpu():
    lib = _lib.load()
    null = ctypes.c_void_p()
    one = ctypes.c_void_p(8)          # never dereferenced: every call below fails its argument check first
    INVALID = _lib.SPDM_ERR_INVALID
    assert lib.spdm_decoder_create(0, null, 4, None, 1, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert lib.spdm_decoder_forward(null, 1, one, one, null) == INVALID
    assert lib.spdm_decoder_forward(one, 0, one, one, null) == INVALID
    assert lib.spdm_decoder_forward(one, 1, null, one, null) == INVALID
    assert lib.spdm_decoder_forward(one, 1, one, null, null) == INVALID
    assert lib.spdm_decoder_train_loss(null, 1, one, one, null, one, null) == INVALID
    assert lib.spdm_decoder_train_loss(one, -2, one, one, null, one, null) == INVALID
    assert lib.spdm_decoder_train_loss(one, 1, null, one, null, one, null) == INVALID
    assert lib.spdm_decoder_train_loss(one, 1, one, null, null, one, null) == INVALID
    assert lib.spdm_decoder_train_loss(one, 1, one, one, one, null, null) == INVALID
    assert lib.spdm_decoder_backward(null, 1, one, one, one, one, null) == INVALID
    assert lib.spdm_decoder_backward(one, 0, one, one, one, one, null) == INVALID
    assert lib.spdm_decoder_backward(one, 1, null, one, one, one, null) == INVALID
    assert lib.spdm_decoder_backward(one, 1, one, null, one, one, null) == INVALID
    assert lib.spdm_decoder_backward(one, 1, one, one, null, one, null) == INVALID
    assert lib.spdm_decoder_backward(one, 1, one, one, one, null, null) == INVALID
    assert lib.spdm_decoder_update_weights(null, one, 4, null) == INVALID
    assert lib.spdm_decoder_update_weights(one, null, 4, null) == INVALID
    lib.spdm_decoder_destroy(null)    # a null handle is ignored
