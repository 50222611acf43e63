"""C ABI of the device optimiser step (include/spdm.h: spdm_adam_workspace_doubles, spdm_adam_step, spdm_adam_norm_index)
and DeviceAdam's argument checks, without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from state_policy_diffusionmodel_amd import _lib

NEW = ("spdm_adam_workspace_doubles", "spdm_adam_step", "spdm_adam_norm_index")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spdm.h")


def _decl(hdr, name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return m.group(1).strip()


def test_header_declares_and_library_exports_the_three_symbols():
    hdr = open(HDR).read()
    lib = _lib.load()
    for name in NEW:
        args = _decl(hdr, name)
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
        n_args = 0 if args == "void" else len(args.split(","))
        assert len(_lib.SYMBOLS[name][1]) == n_args, name
    assert re.search(r"#define\s+SPDM_OPTIM_MAX_SEGMENTS\s+4\b", hdr)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*spdm_optim_segment\s*;", hdr)
    assert m
    fields = [f.split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()]
    assert fields == [f[0] for f in _lib.SpdmOptimSegment._fields_] == ["d_param", "d_grad", "d_exp_avg", "d_exp_avg_sq", "numel"]
    assert ctypes.sizeof(_lib.SpdmOptimSegment) == 40


def test_abi_version_is_still_2():
    assert re.search(r"#define\s+SPDM_ABI_VERSION\s+2\b", open(HDR).read())
    assert _lib.ABI_VERSION == 2 and _lib.load().spdm_abi_version() == 2


def test_workspace_holds_the_norm():
    lib = _lib.load()
    assert lib.spdm_adam_workspace_doubles() > lib.spdm_adam_norm_index() > 0
    assert lib.spdm_adam_norm_index() <= 1024                # one partial per workgroup, at most 1024 workgroups


def _seg(p=16, g=32, m=48, v=64, n=8):
    # never dereferenced: every call below fails its argument check first
    return _lib.SpdmOptimSegment(p, g, m, v, n)


def _call(segs, n=None, step=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, max_norm=0.5, ws=4096):
    lib = _lib.load()
    arr = (_lib.SpdmOptimSegment * max(1, len(segs)))(*segs) if segs is not None else None
    return lib.spdm_adam_step(0, arr, len(segs) if n is None else n, step, lr, b1, b2, eps, max_norm,
                              ctypes.c_void_p(ws), ctypes.c_void_p())


def test_invalid_arguments_without_a_gpu():
    INVALID = _lib.SPDM_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    assert _call(None, n=1) == INVALID                        # null segment table
    assert _call([_seg()], ws=None) == INVALID                # null workspace
    for field in ("p", "g", "m", "v"):
        assert _call([_seg(**{field: None})]) == INVALID, field          # a null pointer in a segment
        assert _call([_seg(**{field: 20})]) == INVALID, field            # ... or one that is not 16-byte aligned
        assert _call([_seg(), _seg(**{field: 24})]) == INVALID, field    # ... in any segment
    assert _call([_seg()], ws=4104) == INVALID
    assert _call([_seg()], n=0) == INVALID
    assert _call([_seg()] * 5) == INVALID
    assert _call([_seg()], n=-1) == INVALID
    assert _call([_seg(n=0)]) == INVALID
    assert _call([_seg(), _seg(n=0)]) == INVALID
    assert _call([_seg()], step=0) == INVALID
    assert _call([_seg()], step=-3) == INVALID
    for bad in (nan, inf, -inf):
        assert _call([_seg()], lr=bad) == INVALID
        assert _call([_seg()], eps=bad) == INVALID
        assert _call([_seg()], b1=bad) == INVALID
        assert _call([_seg()], b2=bad) == INVALID
    for bad in (1.0, 1.5, -0.1):
        assert _call([_seg()], b1=bad) == INVALID
        assert _call([_seg()], b2=bad) == INVALID
    assert _call([_seg()], max_norm=nan) == INVALID
    assert b"adam_step" in _lib.load().spdm_last_error()


def test_device_adam_rejects_what_it_does_not_implement():
    from state_policy_diffusionmodel_amd.optim import DeviceAdam
    assert issubclass(DeviceAdam, torch.optim.Optimizer)
    p = [torch.nn.Parameter(torch.zeros(8))]
    with pytest.raises(ValueError, match="weight"):
        DeviceAdam(p, weight_decay=1e-2)
    with pytest.raises(ValueError, match="amsgrad"):
        DeviceAdam(p, amsgrad=True)
    with pytest.raises(ValueError, match="maximi"):
        DeviceAdam(p, maximize=True)


def test_facades_take_the_keyword():
    import inspect
    from state_policy_diffusionmodel_amd.autoencoder import autoencoder
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    for cls in (Diffusion_DDPM, autoencoder):
        par = inspect.signature(cls.configure_optimizers).parameters["device_optimizer"]
        assert par.default is False
