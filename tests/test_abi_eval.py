"""C ABI of the evaluation entry points (include/spdm.h: spdm_eval_errors, spdm_eval_reduce) and their argument checks,
without a GPU: every call below is refused before the device is touched."""
import ctypes
import os
import re

import pytest

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
ERR_FIELDS = ["B", "H", "D", "n_slots", "seq", "obs_h", "inp_h", "P", "runs", "window_base", "first_traj", "d_pred", "d_truth_pos",
              "d_truth_act", "d_translation", "pos_min", "pos_max", "act_min", "act_max", "d_pos_err", "d_act_err"]
RED_FIELDS = ["N", "C", "runs", "d_err", "d_window_mean", "d_window_std", "d_mean", "d_std", "d_workspace", "workspace_doubles"]
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
            continue
        arr = re.fullmatch(r"(\w+)\[(\d+)\]", var)
        fields.append((arr.group(1), c_types[ctype] * int(arr.group(2))) if arr else (var, c_types[ctype]))
    return fields


def test_header_declares_and_library_exports_the_symbols(lib):
    want = {"spdm_eval_errors": "int32_t device, const spdm_eval_errors_args* a, void* stream",
            "spdm_eval_reduce": "int32_t device, const spdm_eval_reduce_args* a, void* stream",
            "spdm_eval_reduce_workspace_doubles": "int64_t N, int32_t C"}
    for name, sig in want.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", _header())
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1).strip()) == sig
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert lib.spdm_abi_version() == 2                                       # additions only


def test_structs_match_the_header():
    fields = _struct_fields("spdm_eval_errors_args")
    assert [f[0] for f in fields] == ERR_FIELDS
    assert list(_lib.SpdmEvalErrorsArgs._fields_) == fields
    A = _lib.SpdmEvalErrorsArgs
    assert ctypes.sizeof(A) == 160                                           # 10 x 4, 8, 4 x 8, 8 x 8, 2 x 8 (LP64), no padding
    assert A.first_traj.offset == 40 and A.d_pred.offset == 48 and A.pos_min.offset == 80 and A.act_max.offset == 120
    assert A.d_pos_err.offset == 144
    fields = _struct_fields("spdm_eval_reduce_args")
    assert [f[0] for f in fields] == RED_FIELDS
    assert list(_lib.SpdmEvalReduceArgs._fields_) == fields
    R = _lib.SpdmEvalReduceArgs
    assert ctypes.sizeof(R) == 72 and R.d_err.offset == 16 and R.workspace_doubles.offset == 64


def _errors(lib, **kw):
    # 7 rows at 3 runs from trajectory 5: windows 1 .. 3; slot 0 is window 1, three slots.  seq 6 = obs 2 + P 4, H = inp 1 + P.
    # Device pointers that are never dereferenced.
    base = dict(B=7, H=5, D=5, n_slots=3, seq=6, obs_h=2, inp_h=1, P=4, runs=3, window_base=1, first_traj=5, d_pred=4096,
                d_truth_pos=8192, d_truth_act=12288, d_translation=16384, pos_min=-1.0, pos_max=1.0, d_pos_err=20480, d_act_err=24576)
    base.update(kw)
    return lib.spdm_eval_errors(0, ctypes.byref(_lib.SpdmEvalErrorsArgs(**base)), ctypes.c_void_p())


def test_eval_errors_refuses_invalid_arguments_without_a_gpu(lib):
    assert lib.spdm_eval_errors(0, None, ctypes.c_void_p()) == INVALID
    for name in ("d_pred", "d_truth_pos", "d_translation", "d_pos_err"):
        assert _errors(lib, **{name: None}) == INVALID, name
    assert b"null" in lib.spdm_last_error()
    assert _errors(lib, d_truth_act=None) == INVALID                         # the action output needs the action truth
    for name in ("B", "P", "runs", "n_slots", "seq"):
        for bad in (0, -1):
            assert _errors(lib, **{name: bad}) == INVALID, (name, bad)
    assert _errors(lib, H=4) == INVALID and _errors(lib, H=6) == INVALID     # H != inp_h + P
    assert b"inp_h + P" in lib.spdm_last_error()
    assert _errors(lib, D=4) == INVALID                                      # no action columns ...
    assert _errors(lib, D=1, d_act_err=None) == INVALID                      # ... no position columns
    assert _errors(lib, seq=5) == INVALID                                    # seq < obs_h + P
    assert _errors(lib, obs_h=3) == INVALID
    assert _errors(lib, inp_h=3, H=7) == INVALID                             # inp_h > obs_h
    assert _errors(lib, inp_h=-1, H=3) == INVALID
    assert _errors(lib, obs_h=-1, inp_h=0, H=4) == INVALID
    assert _errors(lib, first_traj=-1) == INVALID
    assert _errors(lib, first_traj=2 ** 63 - 3) == INVALID
    assert _errors(lib, window_base=2) == INVALID                            # row 0 is window 1: slot -1
    assert _errors(lib, n_slots=2) == INVALID                                # row 6 is window 3: slot 2
    assert b"n_slots" in lib.spdm_last_error()
    assert _errors(lib, B=8) == INVALID                                      # row 7 is window 4
    assert _errors(lib, first_traj=6) == INVALID                             # rows 6 .. 12 reach window 4
    assert _errors(lib, runs=2) == INVALID                                   # rows 5 .. 11 at 2 runs: windows 2 .. 5
    assert _errors(lib, B=2 ** 30, P=4, n_slots=2 ** 30) == INVALID         # B x P beyond 31 bits
    assert b"eval_errors" in lib.spdm_last_error()


def _reduce(lib, **kw):
    base = dict(N=21, C=4, runs=3, d_err=4096, d_window_mean=8192, d_window_std=12288, d_mean=16384, d_std=20480, d_workspace=24576,
                workspace_doubles=4)
    base.update(kw)
    return lib.spdm_eval_reduce(0, ctypes.byref(_lib.SpdmEvalReduceArgs(**base)), ctypes.c_void_p())


def test_eval_reduce_refuses_invalid_arguments_without_a_gpu(lib):
    assert lib.spdm_eval_reduce(0, None, ctypes.c_void_p()) == INVALID
    for name in ("d_err", "d_window_mean", "d_window_std", "d_mean", "d_std", "d_workspace"):
        assert _reduce(lib, **{name: None}) == INVALID, name
    for name in ("N", "C", "runs"):
        for bad in (0, -1):
            assert _reduce(lib, **{name: bad}) == INVALID, (name, bad)
    assert _reduce(lib, runs=4) == INVALID                                   # 21 rows are not whole windows of 4 runs
    assert b"multiple" in lib.spdm_last_error()
    assert _reduce(lib, C=65536, workspace_doubles=65536) == INVALID
    assert _reduce(lib, workspace_doubles=3) == INVALID                      # one block of rows x 4 columns needs 4
    assert b"workspace" in lib.spdm_last_error()
    assert _reduce(lib, N=1026, workspace_doubles=7) == INVALID              # two blocks of rows x 4 columns need 8


def test_workspace_size(lib):
    ws = lib.spdm_eval_reduce_workspace_doubles
    assert ws(1, 1) == 1 and ws(1024, 3) == 3 and ws(1025, 3) == 6 and ws(200000, 12) == 196 * 12
    assert ws(0, 3) == 0 and ws(5, 0) == 0 and ws(-1, 1) == 0
