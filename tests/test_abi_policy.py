"""C ABI of the closed-loop policy's entry points (include/spdm.h: spdm_policy_push, spdm_policy_window,
spdm_policy_unnormalize) and their argument checks, without a GPU."""
import ctypes
import os
import re

import pytest

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
INVALID = _lib.SPDM_ERR_INVALID
STRUCTS = {
    "push": (_lib.SpdmPolicyPushArgs, 96,                  # 4 x 4, 1 x 8, 9 x 8 (LP64), no padding
             ["E", "L", "img_dtype", "reserved", "n", "d_img_in", "d_pos_in", "d_vel_in", "d_act_in", "d_fill", "d_ring_img",
              "d_ring_pos", "d_ring_vel", "d_ring_act"]),
    "window": (_lib.SpdmPolicyWindowArgs, 200,             # 6 x 4, 1 x 8, 4 x 8, 12 x 8, 5 x 8
               ["E", "L", "obs_h", "step_size", "img_dtype", "stats_f32", "n", "d_ring_img", "d_ring_pos", "d_ring_vel", "d_ring_act",
                "pos_min", "pos_max", "vel_min", "vel_max", "act_min", "act_max", "d_image_out", "d_position_out", "d_velocity_out",
                "d_action_out", "d_translation_out"]),
    "unnormalize": (_lib.SpdmPolicyUnnormalizeArgs, 112,   # 4 x 4, 2 x 8, 8 x 8, 2 x 8
                    ["E", "H", "D", "inp_h", "d_x0", "d_translation", "pos_min", "pos_max", "act_min", "act_max", "d_waypoints",
                     "d_actions"]),
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_header_declares_and_library_exports_the_symbol(name):
    m = re.search(r"\bspdm_policy_%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m
    assert re.sub(r"\s+", " ", m.group(1).strip()) == f"int32_t device, const spdm_policy_{name}_args* a, void* stream"
    res, args = _lib.SYMBOLS["spdm_policy_" + name]
    assert res is ctypes.c_int32 and len(args) == 3
    assert getattr(_lib.load(), "spdm_policy_" + name) is not None
    assert _lib.load().spdm_abi_version() == 2                       # an addition: the version stays


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_matches_the_header(name):
    struct, size, names = STRUCTS[name]
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_policy_%s_args\s*;" % name, _header())
    assert m
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    fields = []
    for decl in (d.strip() for d in m.group(1).split(";")):
        if not decl:
            continue
        ctype, field = decl.replace("const ", "").split(None, 1)
        pointer = "*" in ctype or field.startswith("*")
        arr = re.match(r"(\w+)\[(\d+)\]$", field)
        if arr:
            fields.append((arr.group(1), c_types[ctype] * int(arr.group(2))))
        else:
            fields.append((field.lstrip("* "), ctypes.c_void_p if pointer else c_types[ctype]))
    assert [f[0] for f in fields] == names
    assert list(struct._fields_) == fields
    assert ctypes.sizeof(struct) == size
    at = 0                                                           # no implicit padding anywhere
    for field, ctype in struct._fields_:
        assert getattr(struct, field).offset == at, field
        at += ctypes.sizeof(ctype)
    assert at == size


# device pointers that are never dereferenced: every call below fails its argument check first
def _push(**kw):
    base = dict(E=3, L=6, img_dtype=0, reserved=0, n=7, d_img_in=4096, d_pos_in=8192, d_vel_in=12288, d_act_in=16384, d_fill=20480,
                d_ring_img=24576, d_ring_pos=28672, d_ring_vel=32768, d_ring_act=36864)
    base.update(kw)
    return _lib.load().spdm_policy_push(0, ctypes.byref(_lib.SpdmPolicyPushArgs(**base)), ctypes.c_void_p())


def _window(**kw):
    base = dict(E=3, L=6, obs_h=2, step_size=3, img_dtype=0, stats_f32=0, n=7, d_ring_img=4096, d_ring_pos=8192, d_ring_vel=12288,
                d_ring_act=16384, pos_min=-1.0, pos_max=1.0, d_image_out=20480, d_position_out=24576, d_velocity_out=28672,
                d_action_out=32768, d_translation_out=36864)
    base.update(kw)
    return _lib.load().spdm_policy_window(0, ctypes.byref(_lib.SpdmPolicyWindowArgs(**base)), ctypes.c_void_p())


def _unnormalize(**kw):
    base = dict(E=3, H=9, D=5, inp_h=1, d_x0=4096, d_translation=8192, pos_min=-1.0, pos_max=1.0, d_waypoints=12288, d_actions=16384)
    base.update(kw)
    return _lib.load().spdm_policy_unnormalize(0, ctypes.byref(_lib.SpdmPolicyUnnormalizeArgs(**base)), ctypes.c_void_p())


def test_push_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.spdm_policy_push(0, None, ctypes.c_void_p()) == INVALID
    for name in ("E", "L"):
        for bad in (0, -1):
            assert _push(**{name: bad}) == INVALID, (name, bad)
    assert _push(E=1 << 16, L=1 << 15) == INVALID                        # E x L = 2^31
    assert _push(n=-1) == INVALID
    for bad in (2, -1, 255):
        assert _push(img_dtype=bad) == INVALID, bad
    for name in ("d_img_in", "d_pos_in", "d_vel_in", "d_act_in", "d_fill", "d_ring_img", "d_ring_pos", "d_ring_vel", "d_ring_act"):
        assert _push(**{name: None}) == INVALID, name
    for bad in (4096 + 4, 4096 + 8, 4096 + 1):
        assert _push(d_img_in=bad) == INVALID, bad
        assert _push(d_ring_img=24576 + bad) == INVALID, bad
    assert b"aligned" in lib.spdm_last_error() and b"policy_push" in lib.spdm_last_error()


def test_window_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.spdm_policy_window(0, None, ctypes.c_void_p()) == INVALID
    for name in ("E", "L", "obs_h", "step_size"):
        for bad in (0, -1):
            assert _window(**{name: bad}) == INVALID, (name, bad)
    assert _window(obs_h=3) == INVALID                                   # entries 0, 3, 6: the third is slot 0 again
    assert _window(step_size=6) == INVALID
    assert _window(step_size=0x7fffffff) == INVALID                      # (obs_h - 1) * step_size is evaluated in 64 bits
    assert _window(E=1 << 16, L=1 << 15) == INVALID
    assert _window(E=1 << 20, L=800, obs_h=800, step_size=1) == INVALID  # E x L fits, three slices per frame do not
    assert b"31 bits" in lib.spdm_last_error()
    for bad in (0, -1):
        assert _window(n=bad) == INVALID, bad                            # nothing pushed yet
    assert b"pushed" in lib.spdm_last_error()
    for bad in (2, -1):
        assert _window(img_dtype=bad) == INVALID, bad
    for bad in (4, -1):
        assert _window(stats_f32=bad) == INVALID, bad
    assert _window(d_image_out=None, d_position_out=None, d_velocity_out=None, d_action_out=None, d_translation_out=None) == INVALID
    assert _window(d_ring_img=None) == INVALID
    assert _window(d_ring_pos=None) == INVALID
    assert _window(d_ring_pos=None, d_position_out=None) == INVALID      # the translation reads it too
    assert _window(d_ring_vel=None) == INVALID
    assert _window(d_ring_act=None) == INVALID
    for bad in (4096 + 4, 4096 + 8, 4096 + 1):
        assert _window(d_ring_img=bad) == INVALID, bad
        assert _window(d_image_out=20480 + bad) == INVALID, bad
    assert b"aligned" in lib.spdm_last_error() and b"policy_window" in lib.spdm_last_error()


def test_unnormalize_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.spdm_policy_unnormalize(0, None, ctypes.c_void_p()) == INVALID
    for bad in (0, -1):
        assert _unnormalize(E=bad) == INVALID, bad
    assert _unnormalize(inp_h=-1) == INVALID
    assert _unnormalize(inp_h=9) == INVALID                              # no predicted step left
    assert _unnormalize(H=0, inp_h=0) == INVALID
    assert _unnormalize(D=1) == INVALID
    assert _unnormalize(D=4) == INVALID                                  # actions need columns 2..4
    assert b"action" in lib.spdm_last_error()
    assert _unnormalize(E=1 << 20, H=(1 << 11) + 1) == INVALID           # E x P = 2^31
    for name in ("d_x0", "d_translation", "d_waypoints"):
        assert _unnormalize(**{name: None}) == INVALID, name
    assert b"policy_unnormalize" in lib.spdm_last_error()
