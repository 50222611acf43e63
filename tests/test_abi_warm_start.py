"""C ABI of spdm_policy_warm_start (include/spdm.h) and its argument checks, and the argument checks of the Python keywords
that go with it (``sample(start_step=)``), without a GPU."""
import ctypes
import inspect
import os
import re

import pytest

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
INVALID = _lib.SPDM_ERR_INVALID
SIZE = 120                                                                 # 6 x 4, 3 x 8, 2 x 4, 8 x 8 (LP64), no padding
NAMES = ["E", "H", "D", "inp_h", "step_size", "draw", "delta", "seed", "env_offset", "sa", "sb", "d_prev_x0", "d_prev_translation",
         "d_translation", "d_inpaint", "d_noise_in", "d_x", "d_guess", "d_noise"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_and_library_exports_the_symbol():
    m = re.search(r"\bspdm_policy_warm_start\s*\(([^)]*)\)\s*;", _header())
    assert m
    assert re.sub(r"\s+", " ", m.group(1).strip()) == "int32_t device, const spdm_policy_warm_start_args* a, void* stream"
    res, args = _lib.SYMBOLS["spdm_policy_warm_start"]
    assert res is ctypes.c_int32 and len(args) == 3
    assert _lib.load().spdm_policy_warm_start is not None
    assert _lib.load().spdm_abi_version() == 2                             # an addition: the version stays


def test_struct_matches_the_header():
    struct = _lib.SpdmPolicyWarmStartArgs
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_policy_warm_start_args\s*;", _header())
    assert m
    c_types = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
               "float": ctypes.c_float}
    fields = []
    for decl in (d.strip() for d in m.group(1).split(";")):
        if not decl:
            continue
        ctype, field = decl.replace("const ", "").split(None, 1)
        pointer = "*" in ctype or field.startswith("*")
        fields.append((field.lstrip("* "), ctypes.c_void_p if pointer else c_types[ctype]))
    assert [f[0] for f in fields] == NAMES
    assert list(struct._fields_) == fields
    assert ctypes.sizeof(struct) == SIZE
    at = 0                                                                 # no implicit padding anywhere
    for field, ctype in struct._fields_:
        assert getattr(struct, field).offset == at, field
        at += ctypes.sizeof(ctype)
    assert at == SIZE


def test_the_header_names_the_purpose_and_every_refusal():
    text = re.sub(r"\s+", " ", open(HDR).read().replace(" * ", " "))
    doc = text[text.index("spdm_policy_warm_start builds"):text.index("} spdm_policy_warm_start_args;")]
    assert "counter (k, (uint32)(env_offset + e), draw, 8)" in doc and "4-7 spdm_obs_noise, 8 this entry" in doc
    for phrase in ("NULL args", "a NULL d_prev_x0, d_prev_translation, d_translation or d_x", "E, H or step_size < 1", "D < 2",
                   "inp_h outside [0, H]", "d_inpaint NULL with inp_h > 0 (or set with inp_h == 0)", "delta < 0",
                   "E x H x D beyond 31 bits", "sa or sb not finite"):
        assert phrase in doc, phrase


# device pointers that are never dereferenced: every call below fails its argument check first
def _call(**kw):
    base = dict(E=3, H=16, D=5, inp_h=1, step_size=3, draw=0, delta=4, seed=11, env_offset=0, sa=0.8, sb=0.6, d_prev_x0=4096,
                d_prev_translation=8192, d_translation=12288, d_inpaint=16384, d_noise_in=None, d_x=20480, d_guess=24576, d_noise=28672)
    base.update(kw)
    return _lib.load().spdm_policy_warm_start(0, ctypes.byref(_lib.SpdmPolicyWarmStartArgs(**base)), ctypes.c_void_p())


def test_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.spdm_policy_warm_start(0, None, ctypes.c_void_p()) == INVALID
    for name in ("d_prev_x0", "d_prev_translation", "d_translation", "d_x"):
        assert _call(**{name: None}) == INVALID, name
    assert b"null pointer" in lib.spdm_last_error() and b"policy_warm_start" in lib.spdm_last_error()
    for name in ("E", "H", "step_size"):
        for bad in (0, -1):
            assert _call(**{name: bad}) == INVALID, (name, bad)
    for bad in (1, 0, -1):
        assert _call(D=bad) == INVALID, bad
    assert b"position" in lib.spdm_last_error()
    for bad in (-1, 17):
        assert _call(inp_h=bad) == INVALID, bad
    assert _call(d_inpaint=None) == INVALID                                # inp_h = 1 needs it
    assert _call(inp_h=0) == INVALID                                       # inp_h = 0 with d_inpaint set
    assert b"d_inpaint" in lib.spdm_last_error()
    assert _call(delta=-1) == INVALID
    assert b"negative" in lib.spdm_last_error()
    assert _call(E=1 << 20, H=1 << 10, D=2) == INVALID                     # E x H x D = 2^31
    assert _call(E=1, H=1 << 30, D=2) == INVALID                           # H x D alone
    assert _call(E=1 << 30, H=1 << 30, D=1 << 30) == INVALID               # the product is evaluated in 64 bits, factor by factor
    assert b"31 bits" in lib.spdm_last_error()
    for name in ("sa", "sb"):
        for bad in (float("inf"), float("-inf"), float("nan")):
            assert _call(**{name: bad}) == INVALID, (name, bad)
    assert b"finite" in lib.spdm_last_error()


def test_plan_and_sample_take_the_new_keywords_last():
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy, Plan
    par = inspect.signature(SpdmEngine.sample).parameters
    assert list(par)[-1] == "start_step" and par["start_step"].default == 0
    par = inspect.signature(Diffusion_DDPM.sample).parameters
    assert list(par)[-1] == "start_step" and par["start_step"].default == 0 and par["start_step"].kind is inspect.Parameter.KEYWORD_ONLY
    par = inspect.signature(ClosedLoopPolicy.plan).parameters
    assert list(par) == ["self", "seed", "x_T", "warm_start"] and par["warm_start"].default is None
    fields = list(Plan.__dataclass_fields__)
    assert fields == ["waypoints", "actions", "x_0", "steps", "warm"]
    plan = Plan(None, None, None)
    assert plan.steps == 0 and plan.warm is False


def test_sample_refuses_a_start_step_it_cannot_run():
    """The checks come before anything touches the GPU: a model is built (random weights, host side only) and refuses."""
    from state_policy_diffusionmodel_amd.diffusion import load_model
    for kind in ("DDPM", "DDIM"):
        model = load_model(kind, None, None, num_of_ddim_steps=8, model="UNet_FilmnoAttention", noise_steps=8, obs_horizon=2,
                           pred_horizon=15, inpaint_horizon=1, observation_dim=135, prediction_dim=5, step_size=3, weight_seed=3)
        x = object()                                                        # never looked at: the refusal comes first
        for bad in (-1, 8, 9, 1.0, True, None):
            with pytest.raises(ValueError, match="start_step"):
                model.sample({}, batched=True, sharded=False, x_T=x, start_step=bad)
        with pytest.raises(ValueError, match="x_T"):
            model.sample({}, batched=True, sharded=False, start_step=1)
        for option in ("sample_history", "sample_history_stream"):
            with pytest.raises(ValueError, match="sample_history"):
                model.sample({}, option, batched=True, sharded=False, x_T=x, start_step=1)
        with pytest.raises(ValueError, match="sharded"):
            model.sample({}, batched=True, sharded=True, x_T=x, start_step=1)
