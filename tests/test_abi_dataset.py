"""C ABI of the device dataset gather (include/spdm.h: spdm_dataset_gather) and its argument checks, without a GPU."""
import ctypes
import os
import re

import numpy as np

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
FIELDS = ["T", "n_windows", "B", "seq_len", "step_size", "n_frames", "img_dtype", "reserved", "d_img", "d_position", "d_velocity",
          "d_action", "d_window_start", "h_window_start", "d_window_id", "pos_min", "pos_max", "d_image_out", "d_position_out",
          "d_velocity_out", "d_action_out", "d_translation_out", "d_start_out", "d_bad"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_and_library_exports_the_symbol():
    m = re.search(r"\bspdm_dataset_gather\s*\(([^)]*)\)\s*;", _header())
    assert m
    assert re.sub(r"\s+", " ", m.group(1).strip()) == "int32_t device, const spdm_dataset_gather_args* a, void* stream"
    res, args = _lib.SYMBOLS["spdm_dataset_gather"]
    assert res is ctypes.c_int32 and len(args) == 3
    assert _lib.load().spdm_dataset_gather is not None


def test_struct_matches_the_header():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_dataset_gather_args\s*;", _header())
    assert m
    c_types = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    fields = []
    for decl in (d.strip() for d in m.group(1).split(";")):
        if not decl:
            continue
        ctype, name = decl.replace("const ", "").split(None, 1)
        pointer = "*" in ctype or name.startswith("*")
        fields.append((name.lstrip("* "), ctypes.c_void_p if pointer else c_types[ctype]))
    assert [f[0] for f in fields] == FIELDS
    assert list(_lib.SpdmDatasetGatherArgs._fields_) == fields
    assert ctypes.sizeof(_lib.SpdmDatasetGatherArgs) == 160           # 8 x 4, 7 x 8, 2 x 8, 7 x 8 (LP64), no padding
    assert _lib.SpdmDatasetGatherArgs.d_img.offset == 32 and _lib.SpdmDatasetGatherArgs.pos_min.offset == 88


TABLE = np.array([0, 5, 110], dtype=np.int32)       # T = 140, seq 6, step 5: the last legal start is 140 - 1 - 25 = 114


def _call(table=TABLE, **kw):
    # device pointers that are never dereferenced: every call below fails its argument check first
    base = dict(T=140, n_windows=3, B=2, seq_len=6, step_size=5, n_frames=2, img_dtype=0, reserved=0, d_img=4096, d_position=8192,
                d_velocity=12288, d_action=16384, d_window_start=20480, h_window_start=table.ctypes.data, d_window_id=24576,
                pos_min=-1.0, pos_max=1.0, d_image_out=28672, d_position_out=32768, d_velocity_out=36864, d_action_out=40960,
                d_translation_out=None, d_start_out=None, d_bad=None)
    base.update(kw)
    return _lib.load().spdm_dataset_gather(0, ctypes.byref(_lib.SpdmDatasetGatherArgs(**base)), ctypes.c_void_p())


def test_invalid_arguments_without_a_gpu():
    INVALID = _lib.SPDM_ERR_INVALID
    lib = _lib.load()
    assert lib.spdm_dataset_gather(0, None, ctypes.c_void_p()) == INVALID
    for name in ("seq_len", "step_size", "B", "T", "n_windows"):
        for bad in (0, -1):
            assert _call(**{name: bad}) == INVALID, (name, bad)
    assert _call(n_frames=7) == INVALID                                  # > seq_len
    assert _call(n_frames=-1) == INVALID
    for bad in (2, -1, 255):
        assert _call(img_dtype=bad) == INVALID, bad
    for bad in (4096 + 4, 4096 + 8, 4096 + 1):
        assert _call(d_img=bad) == INVALID, bad                          # a misaligned image base
        assert _call(d_image_out=bad) == INVALID, bad
    assert b"aligned" in lib.spdm_last_error()
    assert _call(table=np.array([0, 5, 115], dtype=np.int32)) == INVALID     # 115 + 25 = 140: one row past the stores
    assert b"window 2" in lib.spdm_last_error()
    assert _call(table=np.array([0, -1, 110], dtype=np.int32)) == INVALID
    assert _call(T=135) == INVALID                                       # the same table against a shorter store
    assert _call(T=20) == INVALID                                        # no window fits at all
    assert _call(step_size=0x7fffffff) == INVALID                        # (seq_len - 1) * step_size is evaluated in 64 bits
    assert _call(d_window_id=None) == INVALID
    assert _call(h_window_start=None) == INVALID                         # a device table needs its host copy, and the reverse
    assert _call(d_window_start=None) == INVALID
    assert _call(d_window_start=None, h_window_start=None, n_windows=116) == INVALID      # identity table: at most 115 starts
    assert _call(d_image_out=None) == INVALID                            # n_frames > 0 without an output
    assert _call(n_frames=0) == INVALID                                  # ... and the reverse
    assert _call(d_img=None) == INVALID
    assert _call(d_position=None) == INVALID
    assert _call(d_position=None, d_position_out=None, d_translation_out=64) == INVALID
    assert _call(d_velocity=None) == INVALID
    assert _call(d_action=None) == INVALID
    assert b"dataset_gather" in lib.spdm_last_error()
