"""C ABI of spdm_policy_select (include/spdm.h) and its argument checks, and the argument checks of the Python keywords that go
with it (``sample(candidates=)``, ``plan_candidates(candidates=, select=, cols=)``), without a GPU."""
import ctypes
import inspect
import os
import re

import pytest

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
INVALID = _lib.SPDM_ERR_INVALID
SIZE = 112                                                                 # 8 x 4, 1 x 8, 3 x 8, 2 x 8, 4 x 8 (LP64), no padding
NAMES = ["E", "K", "H", "D", "inp_h", "cols", "mode", "rows", "guess_row_stride", "d_x0", "d_guess", "d_translation", "pos_min", "pos_max",
         "d_chosen", "d_x0_out", "d_scores", "d_spread"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_and_library_exports_the_symbol():
    m = re.search(r"\bspdm_policy_select\s*\(([^)]*)\)\s*;", _header())
    assert m
    assert re.sub(r"\s+", " ", m.group(1).strip()) == "int32_t device, const spdm_policy_select_args* a, void* stream"
    res, args = _lib.SYMBOLS["spdm_policy_select"]
    assert res is ctypes.c_int32 and len(args) == 3
    assert _lib.load().spdm_policy_select is not None
    assert _lib.load().spdm_abi_version() == 2                             # an addition: the version stays
    m = re.search(r"enum\s*\{\s*SPDM_SELECT_MEDOID\s*=\s*(\d+)\s*,\s*SPDM_SELECT_COHERENT\s*=\s*(\d+)\s*\}", _header())
    assert m and (int(m.group(1)), int(m.group(2))) == (_lib.SPDM_SELECT_MEDOID, _lib.SPDM_SELECT_COHERENT) == (0, 1)


def test_struct_matches_the_header():
    struct = _lib.SpdmPolicySelectArgs
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_policy_select_args\s*;", _header())
    assert m
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
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


def test_the_header_states_the_arithmetic_and_every_refusal():
    text = re.sub(r"\s+", " ", open(HDR).read().replace(" * ", " "))
    doc = text[text.index("spdm_policy_select keeps"):text.index("} spdm_policy_select_args;")]
    for phrase in ("ONE launch", "no atomics", "candidate k of environment e is row e K + k", "d(j,j) is included",
                   "the smallest j whose s_j is minimal", "A NaN score never wins against a non-NaN one", "the choice is 0",
                   "square u, square v, add", "the correctly rounded one"):
        assert phrase in doc, phrase
    for phrase in ("NULL args", "a NULL d_x0, d_chosen or d_x0_out", "E < 1", "K outside [1, 64]", "inp_h < 0 or H <= inp_h", "D < 2",
                   "cols outside [2, D]", "an unknown mode", "COHERENT with a NULL d_guess, rows outside [1, P] or guess_row_stride < 1",
                   "MEDOID with a d_guess or rows != 0", "d_spread without d_translation", "E x K x H x D beyond 31 bits"):
        assert phrase in doc, phrase


# device pointers that are never dereferenced: every call below fails its argument check first
def _call(**kw):
    base = dict(E=3, K=5, H=16, D=5, inp_h=1, cols=2, mode=_lib.SPDM_SELECT_COHERENT, rows=4, guess_row_stride=1, d_x0=1 << 20,
                d_guess=2 << 20, d_translation=3 << 20, pos_min=-1.0, pos_max=1.0, d_chosen=4 << 20, d_x0_out=5 << 20, d_scores=6 << 20,
                d_spread=7 << 20)
    base.update(kw)
    return _lib.load().spdm_policy_select(0, ctypes.byref(_lib.SpdmPolicySelectArgs(**base)), ctypes.c_void_p())


MEDOID = dict(mode=_lib.SPDM_SELECT_MEDOID, d_guess=None, rows=0)


def test_invalid_arguments_without_a_gpu():
    lib = _lib.load()

    def refused(word, **kw):
        assert _call(**kw) == INVALID, kw
        msg = lib.spdm_last_error()
        assert b"policy_select" in msg and word in msg, (kw, msg)

    assert lib.spdm_policy_select(0, None, ctypes.c_void_p()) == INVALID
    assert b"policy_select" in lib.spdm_last_error() and b"null argument" in lib.spdm_last_error()
    for name in ("d_x0", "d_chosen", "d_x0_out"):
        refused(b"null pointer", **{name: None})
        refused(b"null pointer", **{name: None}, **MEDOID)
    for bad in (0, -1):
        refused(b"E =", E=bad)
    for bad in (0, -1, 65, 1 << 20):
        refused(b"K =", K=bad)
    for bad in (-1, 16, 17):
        refused(b"inp_h", inp_h=bad)
    refused(b"inp_h", H=0, inp_h=0)
    for bad in (1, 0, -1):
        refused(b"position", D=bad)
    for bad in (1, 0, -1, 6):
        refused(b"cols", cols=bad)
    refused(b"cols", D=2, cols=3)
    for bad in (2, -1, 7):
        refused(b"mode", mode=bad)
    refused(b"d_guess", d_guess=None)                                      # COHERENT needs it
    for bad in (0, -1, 16):                                                # H - inp_h = 15
        refused(b"rows", rows=bad)
    for bad in (0, -1, -(1 << 40)):
        refused(b"guess_row_stride", guess_row_stride=bad)
    refused(b"MEDOID", mode=_lib.SPDM_SELECT_MEDOID, rows=0)               # a guess is given
    refused(b"MEDOID", mode=_lib.SPDM_SELECT_MEDOID, d_guess=None)         # rows = 4
    refused(b"d_translation", d_translation=None)
    refused(b"d_translation", d_translation=None, **MEDOID)
    refused(b"31 bits", E=1 << 15, K=64, H=1 << 10, D=2, rows=1)           # E x K x H x D = 2^32
    refused(b"31 bits", E=1 << 14, K=64, H=1 << 10, D=2, rows=1)           # 2^31
    refused(b"31 bits", E=1, K=1, H=1 << 30, D=2, rows=1)                  # H x D alone
    refused(b"31 bits", E=(1 << 31) - 1, K=64, H=(1 << 31) - 1, D=(1 << 31) - 1, cols=2, rows=1)        # evaluated in 64 bits, by factors
    refused(b"overlaps", d_x0_out=(1 << 20) + 4)                           # inside d_x0
    # the extremes that are valid fail later, not here: K = 1 and K = 64, rows = 15, cols = D, no optional output -- not called, since
    # a valid call would touch the GPU


def test_sample_and_plan_candidates_take_the_new_keywords():
    import dataclasses
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    from state_policy_diffusionmodel_amd.policy import CandidatePlan, ClosedLoopPolicy, Plan
    par = inspect.signature(Diffusion_DDPM.sample).parameters
    assert par["candidates"].default == 1 and par["candidates"].kind is inspect.Parameter.KEYWORD_ONLY
    # plan() and Plan stay what they were; the candidates come through a method and a result type of their own
    par = inspect.signature(ClosedLoopPolicy.plan_candidates).parameters
    assert list(par) == list(inspect.signature(ClosedLoopPolicy.plan).parameters) + ["candidates", "select", "cols"]
    assert (par["candidates"].default, par["select"].default, par["cols"].default) == (1, "coherent", 2)
    assert issubclass(CandidatePlan, Plan)
    assert [f.name for f in dataclasses.fields(CandidatePlan)] == [f.name for f in dataclasses.fields(Plan)] + [
        "candidates", "selected_by", "chosen", "scores", "spread"]
    plan = CandidatePlan(None, None, None)
    assert (plan.steps, plan.warm, plan.candidates, plan.selected_by, plan.chosen, plan.scores, plan.spread) == (0, False, 1, "", None, None, None)


def test_sample_refuses_candidates_it_cannot_run():
    """The checks come before anything touches the GPU: a model is built (random weights, host side only) and refuses."""
    from state_policy_diffusionmodel_amd.diffusion import load_model
    model = load_model("DDIM", None, None, num_of_ddim_steps=8, model="UNet_FilmnoAttention", noise_steps=8, obs_horizon=2, pred_horizon=15,
                       inpaint_horizon=1, observation_dim=135, prediction_dim=5, step_size=3, weight_seed=3)
    for bad in (0, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="candidates"):
            model.sample({}, batched=True, sharded=False, candidates=bad)
    with pytest.raises(ValueError, match="batched=True"):
        model.sample({}, candidates=2)
    with pytest.raises(ValueError, match="sharded"):
        model.sample({}, batched=True, sharded=True, candidates=2)
    for option in ("sample_history", "sample_history_stream"):
        with pytest.raises(ValueError, match="sample_history"):
            model.sample({}, option, batched=True, sharded=False, candidates=2)


def test_the_command_line_takes_the_new_options():
    from state_policy_diffusionmodel_amd.run_predictions import parse_arguments
    need = ["--checkpoint", "c", "--hparams", "h", "--stats", "s", "--data", "d"]
    args = parse_arguments(need)
    assert (args.candidates, args.select, args.select_cols) == (1, "coherent", 2)
    args = parse_arguments(need + ["--candidates", "16", "--select", "first", "--select_cols", "5"])
    assert (args.candidates, args.select, args.select_cols) == (16, "first", 5)
    with pytest.raises(SystemExit):
        parse_arguments(need + ["--select", "best"])
