"""C ABI of spdm_obs_noise (include/spdm.h) and its argument checks, and the argument checks of evaluation.robustness, without
a GPU: every call below is refused before the device is touched."""
import ctypes
import os
import re

import pytest

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
INVALID = _lib.SPDM_ERR_INVALID
C_TYPES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "spdm_obs_noise_tensor": _lib.SpdmObsNoiseTensor}


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
    fields = []
    for decl in (d.strip() for d in m.group(1).split(";")):
        if not decl:
            continue
        ctype, var = decl.replace("const ", "").split(None, 1)
        if "*" in ctype or var.startswith("*"):
            fields.append((var.lstrip("* "), ctypes.c_void_p))
            continue
        arr = re.fullmatch(r"(\w+)\[(\d+)\]", var)
        fields.append((arr.group(1), C_TYPES[ctype] * int(arr.group(2))) if arr else (var, C_TYPES[ctype]))
    return fields


def test_header_declares_and_library_exports_the_symbol(lib):
    m = re.search(r"\bspdm_obs_noise\s*\(([^)]*)\)\s*;", _header())
    assert m and re.sub(r"\s+", " ", m.group(1).strip()) == "int32_t device, const spdm_obs_noise_args* a, void* stream"
    assert "spdm_obs_noise" in _lib.SYMBOLS and lib.spdm_obs_noise is not None
    assert lib.spdm_abi_version() == 2                                       # an addition only


def test_structs_match_the_header():
    T, A = _lib.SpdmObsNoiseTensor, _lib.SpdmObsNoiseArgs
    assert list(T._fields_) == _struct_fields("spdm_obs_noise_tensor")
    assert ctypes.sizeof(T) == 40 and T.inner.offset == 16                   # 2 pointers, 3 x 8 (LP64), no padding
    fields = _struct_fields("spdm_obs_noise_args")
    assert [f[0] for f in fields] == ["n_rows", "row_offset", "seed", "draw", "alpha", "n_tensors", "reserved", "tensors"]
    assert [(n, t) for n, t in A._fields_[:-1]] == fields[:-1]
    assert A._fields_[-1][1]._type_ is T and A._fields_[-1][1]._length_ == 4 and fields[-1][1]._length_ == 4
    assert ctypes.sizeof(A) == 40 + 4 * 40 and A.draw.offset == 24 and A.alpha.offset == 28 and A.tensors.offset == 40


def _call(lib, tensors=None, **kw):
    # 5 rows from row 7; frames, position, velocity, action of obs 2 out of windows of 5 rows.  Device pointers that are never
    # dereferenced.
    base = dict(n_rows=5, row_offset=7, seed=11, draw=1, alpha=0.05, n_tensors=4, reserved=0)
    base.update(kw)
    a = _lib.SpdmObsNoiseArgs(**base)
    default = [dict(d_src=4096, d_dst=8192, inner=2 * 27648, src_stride=2 * 27648, dst_stride=2 * 27648),
               dict(d_src=12288, d_dst=16384, inner=4, src_stride=10, dst_stride=4),
               dict(d_src=20480, d_dst=20480, inner=4, src_stride=10, dst_stride=10),
               dict(d_src=24576, d_dst=28672, inner=6, src_stride=15, dst_stride=6)]
    for i, t in enumerate(default if tensors is None else tensors):
        a.tensors[i] = _lib.SpdmObsNoiseTensor(**t)
    return lib.spdm_obs_noise(0, ctypes.byref(a), ctypes.c_void_p())


def _one(lib, **kw):
    t = dict(d_src=4096, d_dst=8192, inner=6, src_stride=15, dst_stride=6)
    t.update(kw)
    return _call(lib, tensors=[t], n_tensors=1)


def test_obs_noise_refuses_invalid_arguments_without_a_gpu(lib):
    assert lib.spdm_obs_noise(0, None, ctypes.c_void_p()) == INVALID
    for bad in (0, -1):
        assert _call(lib, n_rows=bad) == INVALID, bad
    assert b"n_rows" in lib.spdm_last_error()
    for bad in (0, -1, 5):
        assert _call(lib, n_tensors=bad) == INVALID, bad
    assert b"n_tensors" in lib.spdm_last_error()
    assert _one(lib, inner=-1) == INVALID
    assert b"negative" in lib.spdm_last_error()
    assert _one(lib, src_stride=5) == INVALID and _one(lib, dst_stride=5) == INVALID          # a stride below inner
    assert b"strides" in lib.spdm_last_error()
    big = 4 * (2 ** 32 - 1)                                                                   # inner / 4 + 1 = 2^32
    assert _one(lib, inner=big, src_stride=big, dst_stride=big) == INVALID
    assert b"quads" in lib.spdm_last_error()
    assert _call(lib, row_offset=-1) == INVALID
    assert _call(lib, row_offset=2 ** 32 - 4) == INVALID                                      # rows up to 2^32 + 1
    assert _call(lib, n_rows=2 ** 32 + 1, row_offset=0) == INVALID
    assert b"32 bits" in lib.spdm_last_error()
    assert _one(lib, d_src=None) == INVALID and _one(lib, d_dst=None) == INVALID
    assert b"null" in lib.spdm_last_error()
    for bad in (-0.01, float("inf"), float("nan")):
        assert _call(lib, alpha=bad) == INVALID, bad
    assert b"alpha" in lib.spdm_last_error()
    # the second tensor is checked like the first
    two = [dict(d_src=4096, d_dst=8192, inner=4, src_stride=4, dst_stride=4), dict(d_src=4096, d_dst=None, inner=4, src_stride=4, dst_stride=4)]
    assert _call(lib, tensors=two, n_tensors=2) == INVALID
    # a grid beyond 2^31 - 1 workgroups: 2^32 rows of 2^20 quads
    assert _call(lib, tensors=[dict(d_src=4096, d_dst=8192, inner=2 ** 22, src_stride=2 ** 22, dst_stride=2 ** 22)], n_tensors=1,
                 n_rows=2 ** 32, row_offset=0) == INVALID
    assert b"workgroups" in lib.spdm_last_error()


def test_robustness_refuses_bad_arguments_before_it_touches_the_device():
    from state_policy_diffusionmodel_amd.dataset import DeviceDataset
    from state_policy_diffusionmodel_amd.evaluation import robustness
    with pytest.raises(TypeError, match="DeviceDataset"):
        robustness(None, object())
    ds = object.__new__(DeviceDataset)                                       # never initialised: the checks below come first
    with pytest.raises(ValueError, match="draw"):
        robustness(None, ds, levels=(0.0, 0.05), draws=(0,))
    with pytest.raises(ValueError, match="draw"):
        robustness(None, ds, levels=())
    with pytest.raises(ValueError, match=">= 0"):
        robustness(None, ds, levels=(0.0, -0.01))
    with pytest.raises(ValueError, match="finite"):
        robustness(None, ds, levels=(float("nan"),))
    with pytest.raises(ValueError, match="draws"):
        robustness(None, ds, levels=(0.1,), draws=(-1,))
    with pytest.raises(ValueError, match="draws"):
        robustness(None, ds, levels=(0.1,), draws=(2 ** 32,))
