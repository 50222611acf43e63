"""C ABI of the autoencoder's validation and report launches (include/spdm.h: spdm_recon_terms, spdm_frames_to_bytes) and their
argument checks, without a GPU: every call below is refused before the device is touched."""
import ctypes
import os
import re

import pytest

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
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
    want = {"spdm_recon_terms": ("int32_t device, const spdm_recon_terms_args* a, void* stream", _lib.SpdmReconTermsArgs),
            "spdm_frames_to_bytes": ("int32_t device, const spdm_frames_to_bytes_args* a, void* stream", _lib.SpdmFramesToBytesArgs)}
    for name, (sig, struct) in want.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", _header())
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1).strip()) == sig
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int32 and args[0] is ctypes.c_int32 and args[1]._type_ is struct and args[2] is ctypes.c_void_p
        assert getattr(lib, name) is not None
    assert lib.spdm_abi_version() == 2 and _lib.ABI_VERSION == 2            # additions only


def test_structs_match_the_header():
    fields = _struct_fields("spdm_recon_terms_args")
    assert [f[0] for f in fields] == ["n", "reserved", "d_recon", "d_target", "slot_offset", "n_slots", "d_terms"]
    A = _lib.SpdmReconTermsArgs
    assert list(A._fields_) == fields
    assert ctypes.sizeof(A) == 48                                            # 2 x 4, 2 x 8, 2 x 8, 8 (LP64), no padding
    assert A.d_recon.offset == 8 and A.d_target.offset == 16 and A.slot_offset.offset == 24 and A.n_slots.offset == 32
    assert A.d_terms.offset == 40

    fields = _struct_fields("spdm_frames_to_bytes_args")
    assert [f[0] for f in fields] == ["n", "cols", "tile_offset", "n_tiles", "d_frames", "d_out"]
    A = _lib.SpdmFramesToBytesArgs
    assert list(A._fields_) == fields
    assert ctypes.sizeof(A) == 40                                            # 2 x 4, 2 x 8, 2 x 8
    assert A.tile_offset.offset == 8 and A.n_tiles.offset == 16 and A.d_frames.offset == 24 and A.d_out.offset == 32


def _terms(lib, **kw):
    # 5 frames into slots 3 .. 7 of 8.  Device pointers that are never dereferenced.
    base = dict(n=5, reserved=0, d_recon=4096, d_target=1 << 20, slot_offset=3, n_slots=8, d_terms=1 << 21)
    base.update(kw)
    return lib.spdm_recon_terms(0, ctypes.byref(_lib.SpdmReconTermsArgs(**base)), ctypes.c_void_p())


def test_recon_terms_refuses_invalid_arguments_without_a_gpu(lib):
    assert lib.spdm_recon_terms(0, None, ctypes.c_void_p()) == INVALID
    assert b"null" in lib.spdm_last_error()
    for name in ("d_recon", "d_target", "d_terms"):
        assert _terms(lib, **{name: None}) == INVALID, name
        assert b"null" in lib.spdm_last_error()
    for bad in (0, -1):
        assert _terms(lib, n=bad) == INVALID, bad
        assert b">= 1" in lib.spdm_last_error()
    assert _terms(lib, slot_offset=-1) == INVALID
    assert b"negative" in lib.spdm_last_error()
    assert _terms(lib, slot_offset=4) == INVALID                             # 4 + 5 > 8
    assert b"n_slots" in lib.spdm_last_error()
    assert _terms(lib, n_slots=7) == INVALID
    assert _terms(lib, n=9, slot_offset=0) == INVALID                        # more frames than slots
    assert _terms(lib, slot_offset=2 ** 63 - 3, n_slots=2 ** 63 - 1) == INVALID     # no overflow in slot_offset + n
    assert _terms(lib, n_slots=0, slot_offset=0) == INVALID
    for name in ("d_recon", "d_target"):
        for off in (4, 8, 1):
            assert _terms(lib, **{name: 4096 + off}) == INVALID, (name, off)
            assert b"16-byte aligned" in lib.spdm_last_error()
    assert b"recon_terms" in lib.spdm_last_error()


def _u8(lib, **kw):
    # 3 frames into tiles 2 .. 4 of 7, three tiles per row
    base = dict(n=3, cols=3, tile_offset=2, n_tiles=7, d_frames=4096, d_out=1 << 20)
    base.update(kw)
    return lib.spdm_frames_to_bytes(0, ctypes.byref(_lib.SpdmFramesToBytesArgs(**base)), ctypes.c_void_p())


def test_frames_to_u8_refuses_invalid_arguments_without_a_gpu(lib):
    assert lib.spdm_frames_to_bytes(0, None, ctypes.c_void_p()) == INVALID
    assert b"null" in lib.spdm_last_error()
    for name in ("d_frames", "d_out"):
        assert _u8(lib, **{name: None}) == INVALID, name
        assert b"null" in lib.spdm_last_error()
        for off in (1, 4, 8):
            assert _u8(lib, **{name: 4096 + off}) == INVALID, (name, off)
            assert b"16-byte aligned" in lib.spdm_last_error()
    for name in ("n", "cols", "n_tiles"):
        for bad in (0, -1):
            assert _u8(lib, **{name: bad}) == INVALID, (name, bad)
            assert b">= 1" in lib.spdm_last_error()
    assert _u8(lib, tile_offset=-1) == INVALID
    assert b"negative" in lib.spdm_last_error()
    assert _u8(lib, tile_offset=5) == INVALID                                # 5 + 3 > 7
    assert b"n_tiles" in lib.spdm_last_error()
    assert _u8(lib, n_tiles=4) == INVALID
    assert _u8(lib, tile_offset=2 ** 63 - 2, n_tiles=2 ** 63 - 1) == INVALID        # no overflow in tile_offset + n
    assert b"frames_to_u8" in lib.spdm_last_error()
