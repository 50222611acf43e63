"""CPU suite for the in-place weight update: spdm_update_weights and spdm_debug_weight_digest are declared in
include/spdm.h with the argument counts _lib.SYMBOLS binds, and refuse a null handle without touching a GPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from state_policy_diffusionmodel_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from state_policy_diffusionmodel_amd import build
    build.build()
    return _lib.load()


def _declared_args(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spdm.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} not declared in spdm.h"
    return [a for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name,nargs", [("spdm_update_weights", 4), ("spdm_debug_weight_digest", 2)])
def test_declared_with_bound_argument_count(lib, name, nargs):
    assert len(_declared_args(name)) == nargs
    assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_null_handle_is_invalid(lib):
    buf = (ctypes.c_float * 4)()
    assert lib.spdm_update_weights(None, buf, 4, None) == -1
    assert lib.spdm_update_weights(None, None, 0, None) == -1
    d = ctypes.c_uint64(0)
    assert lib.spdm_debug_weight_digest(None, ctypes.byref(d)) == -1
    assert lib.spdm_debug_plan_routes(None, 1, (ctypes.c_int32 * 42)(), 42) == _lib.SPDM_ERR_INVALID
    assert b"null" in lib.spdm_last_error()
