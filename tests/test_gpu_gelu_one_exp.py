"""The device GELU (csrc/device_utils.h gelu_erf: one exponential, coefficients from tools/fit_gelu.py) against float64
torch.nn.functional.gelu, through spdm_op_gelu."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 6e-7          # tests/test_gpu_ops.py's bound for the form this replaces


def device_gelu(x):
    from state_policy_diffusionmodel_amd import _lib
    lib = _lib.load()
    xd = x.float().contiguous().cuda()
    yd = torch.full_like(xd, float("nan"))
    _lib.check(lib.spdm_op_gelu(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(yd.data_ptr()), xd.numel(),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "spdm_op_gelu")
    torch.cuda.synchronize()
    return xd.cpu(), yd.cpu()


def max_err(x):
    x32, y = device_gelu(x)
    want = torch.nn.functional.gelu(x32.double())
    err = float((y.double() - want).abs().max())
    print(f"max |device gelu - fp64| = {err:.3e} on [{float(x32.min()):g}, {float(x32.max()):g}], {x32.numel()} points")
    return err


def test_gelu_on_the_working_range():
    assert max_err(torch.linspace(-12.0, 12.0, 2_000_000, dtype=torch.float64)) <= BOUND


@pytest.mark.parametrize("lo,hi", [(5.5, 6.5), (-6.5, -5.5)])
def test_gelu_across_the_clamp_knee(lo, hi):
    assert max_err(torch.linspace(lo, hi, 100_000, dtype=torch.float64)) <= BOUND


def test_gelu_far_outside_the_clamp():
    x32, y = device_gelu(torch.tensor([6.0, -6.0, 100.0, -100.0, 4000.0, -4000.0]))
    want = torch.nn.functional.gelu(x32.double())
    err = (y.double() - want).abs()
    bound = 1e-6 * x32.double().abs().clamp_min(1.0)
    print("errors", err.tolist())
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())


def test_gelu_propagates_nan():
    """out_step_kernel's non-finite flag relies on a NaN activation staying NaN through the prologue."""
    _, y = device_gelu(torch.tensor([float("nan"), 1.0, -float("nan"), -2.0]))
    assert torch.isnan(y[0]) and torch.isnan(y[2]) and torch.isfinite(y[1]) and torch.isfinite(y[3])
