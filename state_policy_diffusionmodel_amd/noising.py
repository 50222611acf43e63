"""The forward (noising) process of a training step on the device: ``forward_process`` draws the timesteps and the noise,
forms ``x_noisy = sqrt(abar_t) x0 + sqrt(1 - abar_t) noise``, in-paints the observed rows and -- optionally -- draws
simple_Unet.py's time-embedding dropout mask, in ONE HIP launch (``spdm_train_forward_process``).

Replaces the head of the reference's ``training_step`` (models/diffusion_ddpm.py:128-173): ``torch.randint``,
``torch.randn_like``, ``noise_scheduler.add_noise`` and ``add_constraints``.  The randomness is a pure function of
``(seed, step, global sample index)``: Philox4x32-10 streams apart from the sampler's, so a shard of a batch
(``sample_offset = rank * B``, distributed.py's convention) draws exactly what the whole batch would.  Given device
tensors, the call is that one launch on torch's current stream (a host ``t`` or ``noise`` is uploaded first, which waits),
and every result stays on the device."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def forward_process(x0: torch.Tensor, inpaint: Optional[torch.Tensor], sqrt_abar: torch.Tensor, sqrt_1m_abar: torch.Tensor, *,
                    t: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, seed: int = 0, step: int = 0,
                    sample_offset: int = 0, time_dim: Optional[int] = None, dropout_p: Optional[float] = None):
    """``(x_noisy, noise, t)`` -- or ``(x_noisy, noise, t, time_scale)`` when ``time_dim`` and ``dropout_p`` are given.

    ``x0`` (B,H,D) or (B,1,H,D): the clean window, ``torch.cat([x_0_inpaint, x_0], dim=2)``; ``inpaint`` (B|1,[1,]inp_h,D) or
    None: the rows that overwrite ``x_noisy[..., :inp_h, :]``; ``sqrt_abar`` / ``sqrt_1m_abar``: (T,) fp32 device tables
    (``_LinearBetaScheduler.device_tables``).  ``t`` (B,) / ``noise`` (like x0): given values enter the arithmetic in place of
    drawn ones (a ``t`` outside [0, T) is clamped into range on the device).  ``x_noisy`` and ``noise`` come back in x0's
    shape, ``t`` as a device int32 tensor, ``time_scale`` as (B, time_dim): the dropout mask over (1 - p)."""
    if not x0.is_cuda:
        raise ValueError("forward_process runs on the GPU: x0 must be a device tensor (there is no CPU fallback)")
    if x0.dim() not in (3, 4) or (x0.dim() == 4 and x0.shape[1] != 1):
        raise ValueError(f"x0 must be (B,H,D) or (B,1,H,D), got {tuple(x0.shape)}")
    if (time_dim is None) != (dropout_p is None):
        raise ValueError("time_dim and dropout_p go together")
    dev = x0.device
    shape = tuple(x0.shape)
    B, H, D = shape[0], shape[-2], shape[-1]
    xs = _f32(x0, dev).reshape(B, H, D)
    sa, sb = _f32(sqrt_abar, dev).reshape(-1), _f32(sqrt_1m_abar, dev).reshape(-1)
    T = sa.numel()
    if sb.numel() != T:
        raise ValueError("sqrt_abar and sqrt_1m_abar must have the same length")
    ip, inp_h = None, 0
    if inpaint is not None and inpaint.numel() > 0:
        ip = _f32(inpaint, dev)
        ip = ip.reshape(-1, ip.shape[-2], ip.shape[-1])
        inp_h = ip.shape[1]
        if ip.shape[2] != D or ip.shape[0] not in (1, B):
            raise ValueError(f"inpaint must be (1|B,[1,]inp_h,{D}), got {tuple(inpaint.shape)}")
        if ip.shape[0] != B:
            ip = ip.expand(B, inp_h, D).contiguous()
    t_in = n_in = None
    if t is not None:
        t_in = t.detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if t_in.numel() != B:
            raise ValueError(f"t must have B = {B} elements, got {t_in.numel()}")
    if noise is not None:
        if noise.numel() != xs.numel():
            raise ValueError(f"noise must have x0's shape {shape}, got {tuple(noise.shape)}")
        n_in = _f32(noise, dev).reshape(B, H, D)
    t_out = torch.empty(B, device=dev, dtype=torch.int32)
    n_out = n_in if n_in is not None else torch.empty((B, H, D), device=dev, dtype=torch.float32)
    x_noisy = torch.empty((B, H, D), device=dev, dtype=torch.float32)
    ts = torch.empty((B, int(time_dim)), device=dev, dtype=torch.float32) if time_dim is not None else None
    p = lambda v: v.data_ptr() if v is not None else None  # noqa: E731
    a = _lib.SpdmForwardProcessArgs(
        B=B, H=H, D=D, inp_h=inp_h, T=T, time_dim=int(time_dim) if time_dim is not None else 0,
        d_x0=p(xs), d_inpaint=p(ip), d_sqrt_abar=p(sa), d_sqrt_1m_abar=p(sb),
        seed=int(seed) & 0xFFFFFFFFFFFFFFFF, sample_offset=int(sample_offset) & 0xFFFFFFFFFFFFFFFF,
        step=int(step) & 0xFFFFFFFF, dropout_p=float(dropout_p) if dropout_p is not None else 0.0,
        d_t_in=p(t_in), d_noise_in=p(n_in), d_t=p(t_out), d_noise=p(n_out), d_x_noisy=p(x_noisy), d_time_scale=p(ts),
        d_clamped=None)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().spdm_train_forward_process(index, ctypes.byref(a), stream), "spdm_train_forward_process")
    out = (x_noisy.view(shape), n_out.view(shape), t_out)
    return out + (ts,) if ts is not None else out


__all__ = ["forward_process"]
