"""C ABI of the device forward process (include/spdm.h: spdm_train_forward_process, spdm_train_loss_grad_dt) and
training_step's new argument checks, without a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from state_policy_diffusionmodel_amd import _lib

NEW = ("spdm_train_forward_process", "spdm_train_loss_grad_dt")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")
FIELDS = ["B", "H", "D", "inp_h", "T", "time_dim", "d_x0", "d_inpaint", "d_sqrt_abar", "d_sqrt_1m_abar", "seed", "sample_offset",
          "step", "dropout_p", "d_t_in", "d_noise_in", "d_t", "d_noise", "d_x_noisy", "d_time_scale", "d_clamped"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def _decl(hdr, name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return m.group(1).strip()


def test_header_declares_and_library_exports_both_symbols():
    hdr = _header()
    lib = _lib.load()
    for name in NEW:
        args = _decl(hdr, name)
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
        assert len(_lib.SYMBOLS[name][1]) == len(args.split(",")), name
    # the device-t entry takes spdm_train_loss_grad's arguments, the timesteps as a device pointer in the same place
    assert _lib.SYMBOLS["spdm_train_loss_grad_dt"] == _lib.SYMBOLS["spdm_train_loss_grad"]
    a, b = _decl(hdr, "spdm_train_loss_grad_dt"), _decl(hdr, "spdm_train_loss_grad")
    assert re.sub(r"\s+", " ", a).replace("d_t,", "h_t,") == re.sub(r"\s+", " ", b)


def test_struct_matches_the_header():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_forward_process_args\s*;", _header())
    assert m
    c_types = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    fields = []
    for decl in (d.strip() for d in m.group(1).split(";")):
        if not decl:
            continue
        decl = decl.replace("const ", "")
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            n = n.strip()
            pointer = "*" in ctype or n.startswith("*")
            fields.append((n.lstrip("* "), ctypes.c_void_p if pointer else c_types[ctype.rstrip("*")]))
    assert [f[0] for f in fields] == FIELDS
    assert [(n, t) for n, t in _lib.SpdmForwardProcessArgs._fields_] == fields
    assert ctypes.sizeof(_lib.SpdmForwardProcessArgs) == 136          # 6 x 4, 4 x 8, 2 x 8, 2 x 4, 7 x 8 (LP64), no padding
    assert _lib.SpdmForwardProcessArgs.d_x0.offset == 24 and _lib.SpdmForwardProcessArgs.d_t_in.offset == 80


def test_abi_version_is_still_2():
    assert re.search(r"#define\s+SPDM_ABI_VERSION\s+2\b", open(HDR).read())
    assert _lib.ABI_VERSION == 2 and _lib.load().spdm_abi_version() == 2


def _args(**kw):
    # pointers that are never dereferenced: every call below fails its argument check first
    base = dict(B=2, H=4, D=3, inp_h=1, T=10, time_dim=0, d_x0=16, d_inpaint=32, d_sqrt_abar=48, d_sqrt_1m_abar=64, seed=1,
                sample_offset=0, step=0, dropout_p=0.0, d_t_in=None, d_noise_in=None, d_t=80, d_noise=96, d_x_noisy=112,
                d_time_scale=None, d_clamped=None)
    base.update(kw)
    return _lib.SpdmForwardProcessArgs(**base)


def _call(**kw):
    return _lib.load().spdm_train_forward_process(0, ctypes.byref(_args(**kw)), ctypes.c_void_p())


def test_invalid_arguments_without_a_gpu():
    INVALID = _lib.SPDM_ERR_INVALID
    lib = _lib.load()
    assert lib.spdm_train_forward_process(0, None, ctypes.c_void_p()) == INVALID
    for name in ("d_x0", "d_sqrt_abar", "d_sqrt_1m_abar", "d_x_noisy"):
        assert _call(**{name: None}) == INVALID, name                   # a required pointer
    assert _call(d_t=None) == INVALID                                    # drawn t needs its output
    assert _call(d_noise=None) == INVALID                                # drawn noise needs its output
    for name in ("B", "H", "D", "T"):
        for bad in (0, -1):
            assert _call(**{name: bad}) == INVALID, (name, bad)
    assert _call(H=0x7fffffff - 2, D=1) == INVALID                       # H x D rounded up to whole quads must fit an int
    assert _call(H=46341, D=46341) == INVALID
    assert _call(d_time_scale=128, time_dim=0x7fffffff - 2, dropout_p=0.1) == INVALID
    assert _call(inp_h=-1) == INVALID
    assert _call(inp_h=5) == INVALID                                     # > H
    assert _call(d_inpaint=None) == INVALID                              # inp_h > 0 without rows
    for bad in (0, -3):
        assert _call(d_time_scale=128, time_dim=bad, dropout_p=0.1) == INVALID
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        assert _call(dropout_p=bad) == INVALID, bad
        assert _call(d_time_scale=128, time_dim=8, dropout_p=bad) == INVALID, bad
    assert b"forward_process" in lib.spdm_last_error()


def test_device_t_entry_rejects_a_null_handle():
    lib = _lib.load()
    p = ctypes.c_void_p
    assert lib.spdm_train_loss_grad_dt(None, 1, p(16), p(32), 1, None, p(48), p(64), None, p(80), None, p()) == _lib.SPDM_ERR_INVALID
    assert b"null handle" in lib.spdm_last_error()


def test_python_surface():
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    from state_policy_diffusionmodel_amd.noising import forward_process
    from state_policy_diffusionmodel_amd.schedulers import DDPMScheduler
    par = inspect.signature(Diffusion_DDPM.training_step).parameters
    assert par["device_noise"].default is False and par["seed"].default == 0 and par["noise_step"].default is None
    assert par["sample_offset"].default == 0 and par["time_dropout"].default is None
    assert callable(Diffusion_DDPM.forward_process)
    par = inspect.signature(forward_process).parameters
    assert list(par)[:4] == ["x0", "inpaint", "sqrt_abar", "sqrt_1m_abar"]
    for k in ("t", "noise", "seed", "step", "sample_offset", "time_dim", "dropout_p"):
        assert par[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    with pytest.raises(ValueError, match="no CPU fallback"):
        forward_process(torch.zeros(2, 4, 3), None, torch.ones(10), torch.ones(10))
    # the cached tables are add_noise's own expressions
    s = DDPMScheduler(num_train_timesteps=50)
    sa, sb = s.device_tables("cpu")
    assert torch.equal(sa, s.alphas_cumprod ** 0.5) and torch.equal(sb, (1 - s.alphas_cumprod) ** 0.5)
    assert s.device_tables("cpu")[0] is sa


class _Stub:
    """training_step's argument checks come first: they need no engine and no GPU."""
    simple = True

    def __init__(self, simple):
        self.simple = simple


@pytest.mark.parametrize("kw,simple,match", [
    (dict(time_dropout=0.1, backward=True, device_noise=True, time_scale=torch.ones(2, 256)), True, "not both"),
    (dict(time_dropout=0.1, backward=False, device_noise=True), True, "backward=True"),
    (dict(time_dropout=0.1, backward=True, device_noise=True), False, "model='UNet'"),
    (dict(time_dropout=0.1, backward=True, device_noise=False), True, "device_noise=True"),
    (dict(time_dropout=1.0, backward=True, device_noise=True), True, r"\[0, 1\)"),
    (dict(time_dropout=-0.5, backward=True, device_noise=True), True, r"\[0, 1\)"),
])
def test_training_step_rejects_bad_dropout_arguments(kw, simple, match):
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    with pytest.raises(ValueError, match=match):
        Diffusion_DDPM.training_step(_Stub(simple), {}, **kw)
