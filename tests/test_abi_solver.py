"""C ABI of the DPM-Solver++ (2M) additions (include/spdm.h: SPDM_DPMPP_2M, spdm_solver_step) and the argument checks that
come before the GPU is touched.  No GPU."""
import ctypes
import os
import re

import numpy as np

from state_policy_diffusionmodel_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
INVALID = _lib.SPDM_ERR_INVALID
SIZE = 88                                                                  # 8 x 4, 7 x 8 (LP64), no padding
NAMES = ["B", "H", "D", "inp_h", "inpaint_per_sample", "n_steps", "step", "first", "d_eps", "d_x", "d_x0_prev", "d_coef", "d_inpaint",
         "d_history", "d_words"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_and_library_exports_the_symbol():
    m = re.search(r"\bspdm_solver_step\s*\(([^)]*)\)\s*;", _header())
    assert m
    assert re.sub(r"\s+", " ", m.group(1).strip()) == "int32_t device, const spdm_solver_step_args* a, void* stream"
    res, args = _lib.SYMBOLS["spdm_solver_step"]
    assert res is ctypes.c_int32 and len(args) == 3
    assert _lib.load().spdm_solver_step is not None
    assert _lib.load().spdm_abi_version() == 2 == _lib.ABI_VERSION          # an addition: the version stays
    assert re.search(r"#define\s+SPDM_ABI_VERSION\s+2\b", _header())


def test_the_scheduler_kind_is_declared():
    m = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*spdm_scheduler_kind\s*;", _header())
    assert m
    kinds = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert kinds == {"SPDM_DDPM": 0, "SPDM_DDIM": 1, "SPDM_DPMPP_2M": 2}
    assert (_lib.SPDM_DDPM, _lib.SPDM_DDIM, _lib.SPDM_DPMPP_2M) == (0, 1, 2)


def test_struct_matches_the_header():
    struct = _lib.SpdmSolverStepArgs
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_solver_step_args\s*;", _header())
    assert m
    fields = []
    for decl in (d.strip() for d in m.group(1).split(";")):
        if not decl:
            continue
        ctype, field = decl.replace("const ", "").split(None, 1)
        pointer = "*" in ctype or field.startswith("*")
        fields.append((field.lstrip("* "), ctypes.c_void_p if pointer else {"int32_t": ctypes.c_int32}[ctype]))
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
    doc = text[text.index("spdm_solver_step is one DPM-Solver++"):text.index("} spdm_solver_step_args;")]
    for phrase in ("x0 = (x - c0 eps) / c1", "acc = c2 x", "acc + c3 x0", "acc + c4 x0", "acc + c5 x0_prev", "no FMA",
                   "NULL args", "B, H, D or n_steps < 1", "B x H x D beyond 31 bits", "inp_h outside [0, H]",
                   "d_inpaint NULL with inp_h > 0 (or set with inp_h == 0)", "inpaint_per_sample not 0 or 1",
                   "step outside [0, n_steps)", "first outside [-1, n_steps)", "a NULL d_eps, d_x, d_x0_prev, d_coef or d_words"):
        assert phrase in doc, phrase
    sched = text[text.index("SPDM_DPMPP_2M (DPM-Solver++"):text.index("int spdm_set_schedule_tables(")]
    for phrase in ("{ sigma_s, alpha_s, k_x, k0f, k0, k1 }", "always starts first order", "NOT the tail of the whole loop"):
        assert phrase in sched, phrase


# device pointers that are never dereferenced: every call below fails its argument check first
def _call(**kw):
    base = dict(B=3, H=9, D=5, inp_h=1, inpaint_per_sample=0, n_steps=6, step=2, first=-1, d_eps=4096, d_x=8192, d_x0_prev=12288,
                d_coef=16384, d_inpaint=20480, d_history=None, d_words=24576)
    base.update(kw)
    return _lib.load().spdm_solver_step(0, ctypes.byref(_lib.SpdmSolverStepArgs(**base)), ctypes.c_void_p())


def test_invalid_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.spdm_solver_step(0, None, ctypes.c_void_p()) == INVALID
    assert b"solver_step" in lib.spdm_last_error()
    for name in ("d_eps", "d_x", "d_x0_prev", "d_coef", "d_words"):
        assert _call(**{name: None}) == INVALID, name
        assert b"null pointer" in lib.spdm_last_error() and b"solver_step" in lib.spdm_last_error()
    for name in ("B", "H", "D", "n_steps"):
        for bad in (0, -1):
            assert _call(**{name: bad}) == INVALID, (name, bad)
            assert b">= 1" in lib.spdm_last_error()
    for bad in (-1, 10):
        assert _call(inp_h=bad) == INVALID, bad
        assert b"inp_h" in lib.spdm_last_error()
    assert _call(d_inpaint=None) == INVALID                                # inp_h = 1 needs it
    assert _call(inp_h=0) == INVALID                                       # inp_h = 0 with d_inpaint set
    assert b"d_inpaint" in lib.spdm_last_error()
    for bad in (-1, 2):
        assert _call(inpaint_per_sample=bad) == INVALID
    assert b"inpaint_per_sample" in lib.spdm_last_error()
    for bad in (-1, 6, 7):
        assert _call(step=bad) == INVALID, bad
        assert b"step" in lib.spdm_last_error() and b"[0, n_steps = 6)" in lib.spdm_last_error()
    for bad in (-2, 6):
        assert _call(first=bad) == INVALID, bad
        assert b"first" in lib.spdm_last_error()
    assert _call(B=1 << 20, H=1 << 10, D=2, inp_h=1) == INVALID           # B x H x D = 2^31
    assert _call(B=1, H=1 << 30, D=2) == INVALID                           # H x D alone
    assert _call(B=1 << 30, H=1 << 30, D=1 << 30) == INVALID               # evaluated in 64 bits, factor by factor
    assert b"31 bits" in lib.spdm_last_error()


def test_the_tables_entry_takes_kind_2_and_the_built_in_ones_refuse_it():
    lib = _lib.load()
    ts = (ctypes.c_int32 * 4)()
    coef = (ctypes.c_float * 24)()
    assert lib.spdm_schedule_tables(_lib.SPDM_DDIM, 20, 4, 1e-4, 0.02, ts, coef) == 0
    assert lib.spdm_schedule_tables(_lib.SPDM_DPMPP_2M, 20, 4, 1e-4, 0.02, ts, coef) == INVALID
    assert b"kind 2" in lib.spdm_last_error()
    # spdm_set_schedule_tables answers a null handle before it looks at the kind; that it accepts kind 2 on a real handle is
    # tests/test_gpu_solver.py's business, that its check names kinds 0 .. 2 is read from the source here
    assert lib.spdm_set_schedule_tables(None, 2, 4, ts, coef) == INVALID
    src = open(os.path.join(os.path.dirname(HDR), "..", "state_policy_diffusionmodel_amd", "csrc", "spdm_api.hip")).read()
    body = src[src.index('extern "C" int spdm_set_schedule_tables'):]
    body = body[:body.index("\n}\n")]
    assert "kind != SPDM_DPMPP_2M" in body and "install_schedule(h, kind, n, ts, coef)" in body
    body = src[src.index("static int build_schedule"):]
    assert "SPDM_DPMPP_2M" not in body[:body.index("\n}\n")]


def test_the_scheduler_table_has_the_layout_the_library_takes():
    from state_policy_diffusionmodel_amd.schedulers import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(num_train_timesteps=20)
    s.set_timesteps(6)
    tab = s.coefficient_table()
    assert tab.shape == (6, 6) and tab.dtype == np.float32 and tab.flags["C_CONTIGUOUS"]
    a = np.cumprod(1.0 - np.linspace(1e-4, 0.02, 20))
    t = s.timesteps.numpy()
    assert np.array_equal(tab[:, 0], np.sqrt(1.0 - a[t]).astype(np.float32))      # what ClosedLoopPolicy._noise_level reads
    assert np.array_equal(tab[:, 1], np.sqrt(a[t]).astype(np.float32))
