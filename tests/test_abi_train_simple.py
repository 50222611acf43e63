"""include/spdm.h and the ctypes binding agree on SPDM_FLAG_TRAIN_SIMPLE and spdm_train_set_time_scale (no GPU needed)."""
import os
import re

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(__file__), "..", "include", "spdm.h")


def _header() -> str:
    with open(HDR) as fh:
        return fh.read()


def test_train_simple_flag_matches_header():
    m = re.search(r"#define\s+SPDM_FLAG_TRAIN_SIMPLE\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.SPDM_FLAG_TRAIN_SIMPLE == 32


def test_train_simple_flag_is_a_distinct_power_of_two():
    flags = [_lib.SPDM_FLAG_DEBUG_KEEP, _lib.SPDM_FLAG_EXACT_FP32, _lib.SPDM_FLAG_SIMPLE_UNET, _lib.SPDM_FLAG_TRAIN,
             _lib.SPDM_FLAG_TRAIN_ATTENTION, _lib.SPDM_FLAG_TRAIN_SIMPLE]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)


def test_time_scale_entry_point_is_declared_and_bound():
    m = re.search(r"int\s+spdm_train_set_time_scale\s*\(([^)]*)\)\s*;", _header())
    assert m, "spdm_train_set_time_scale is not declared in include/spdm.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert "spdm_train_set_time_scale" in _lib.SYMBOLS
    res, args = _lib.SYMBOLS["spdm_train_set_time_scale"]
    assert n_args == len(args) == 3


def test_train_loss_grad_signature_unchanged():
    m = re.search(r"int\s+spdm_train_loss_grad\s*\(([^)]*)\)\s*;", _header())
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 12
    assert len(_lib.SYMBOLS["spdm_train_loss_grad"][1]) == 12


def test_abi_version_is_still_2():
    m = re.search(r"#define\s+SPDM_ABI_VERSION\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.ABI_VERSION == 2
