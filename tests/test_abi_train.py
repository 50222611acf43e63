"""include/spdm.h and the ctypes binding agree on the training entry point (no GPU needed)."""
import os
import re

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(__file__), "..", "include", "spdm.h")


def _header() -> str:
    with open(HDR) as fh:
        return fh.read()


def test_train_flag_matches_header():
    m = re.search(r"#define\s+SPDM_FLAG_TRAIN\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.SPDM_FLAG_TRAIN
    flags = [_lib.SPDM_FLAG_DEBUG_KEEP, _lib.SPDM_FLAG_EXACT_FP32, _lib.SPDM_FLAG_SIMPLE_UNET, _lib.SPDM_FLAG_TRAIN]
    assert len(set(flags)) == 4 and all(f & (f - 1) == 0 for f in flags)


def test_abi_version_matches_header():
    m = re.search(r"#define\s+SPDM_ABI_VERSION\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.ABI_VERSION == 2


def test_train_symbol_declared_and_bound():
    m = re.search(r"int\s+spdm_train_loss_grad\(([^)]*)\)", _header())
    assert m, "spdm_train_loss_grad not declared"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = _lib.SYMBOLS["spdm_train_loss_grad"]
    assert len(args) == n_args == 12
