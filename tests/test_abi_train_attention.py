"""include/spdm.h and the ctypes binding agree on SPDM_FLAG_TRAIN_ATTENTION (no GPU needed)."""
import os
import re

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(__file__), "..", "include", "spdm.h")


def _header() -> str:
    with open(HDR) as fh:
        return fh.read()


def test_train_attention_flag_matches_header():
    m = re.search(r"#define\s+SPDM_FLAG_TRAIN_ATTENTION\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.SPDM_FLAG_TRAIN_ATTENTION


def test_train_attention_flag_is_a_distinct_power_of_two():
    flags = [_lib.SPDM_FLAG_DEBUG_KEEP, _lib.SPDM_FLAG_EXACT_FP32, _lib.SPDM_FLAG_SIMPLE_UNET, _lib.SPDM_FLAG_TRAIN,
             _lib.SPDM_FLAG_TRAIN_ATTENTION]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)


def test_abi_version_is_still_2():
    m = re.search(r"#define\s+SPDM_ABI_VERSION\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.ABI_VERSION == 2
