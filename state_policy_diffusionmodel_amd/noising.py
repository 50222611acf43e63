"""The forward (noising) process of a training step on the device: ``forward_process`` draws the timesteps and the noise,
forms ``x_noisy = sqrt(abar_t) x0 + sqrt(1 - abar_t) noise``, in-paints the observed rows and -- optionally -- draws
simple_Unet.py's time-embedding dropout mask, in ONE HIP launch (``spdm_train_forward_process``).

Replaces the head of the reference's ``training_step`` (models/diffusion_ddpm.py:128-173): ``torch.randint``,
``torch.randn_like``, ``noise_scheduler.add_noise`` and ``add_constraints``.  The randomness is a pure function of
``(seed, step, global sample index)``: Philox4x32-10 streams apart from the sampler's, so a shard of a batch
(``sample_offset = rank * B``, distributed.py's convention) draws exactly what the whole batch would.  Given device
tensors, the call is that one launch on torch's current stream (a host ``t`` or ``noise`` is uploaded first, which waits),
and every result stays on the device.

``perturb_observations`` adds ``alpha * U[0, 1)`` to the observed part of a batch of windows, as the reference's
evaluation/eval_robustness.py:180-190 does with four ``torch.rand_like``, in ONE HIP launch (``spdm_obs_noise``, DESIGN.md
8.13); its randomness is a pure function of ``(seed, draw, tensor, global row, element)``."""
from __future__ import annotations

import ctypes
import math
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


OBSERVATION_KEYS = ("image", "position", "velocity", "action")      # in this order: Philox purposes 4, 5, 6, 7


def add_uniform_noise(tensors, alpha: float, *, n_rows: int, seed: int = 0, draw: int = 0, row_offset: int = 0) -> None:
    """One ``spdm_obs_noise`` launch on torch's current stream.  ``tensors``: up to four ``(src, dst, inner, src_stride,
    dst_stride)`` with ``src`` / ``dst`` contiguous float32 device tensors read as ``n_rows`` rows of ``*_stride`` elements from
    their first element (``dst`` may be ``src``; a view that starts anywhere is fine): ``dst[row][e] = src[row][e] + alpha *
    u(row_offset + row, e)`` for ``e < inner``, nothing else is read or written.  Tensor ``i`` draws Philox purpose ``4 + i``."""
    tensors = list(tensors)
    if not 1 <= len(tensors) <= 4:
        raise ValueError(f"{len(tensors)} tensors: one launch takes 1 to 4")
    n_rows = int(n_rows)
    if n_rows < 1:
        raise ValueError(f"n_rows = {n_rows} must be >= 1")
    dev = tensors[0][0].device
    if dev.type != "cuda":
        raise ValueError("add_uniform_noise runs on the GPU: it takes device tensors (there is no CPU fallback)")
    a = _lib.SpdmObsNoiseArgs(n_rows=n_rows, row_offset=int(row_offset), seed=int(seed) & 0xFFFFFFFFFFFFFFFF, draw=int(draw) & 0xFFFFFFFF,
                              alpha=float(alpha), n_tensors=len(tensors), reserved=0)
    for i, (src, dst, inner, src_stride, dst_stride) in enumerate(tensors):
        inner, src_stride, dst_stride = int(inner), int(src_stride), int(dst_stride)
        if inner < 0 or src_stride < inner or dst_stride < inner:
            raise ValueError(f"tensor {i}: inner = {inner} must be >= 0 and at most the strides {src_stride} and {dst_stride}")
        for name, t, stride in (("src", src, src_stride), ("dst", dst, dst_stride)):
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"tensor {i}: {name} must be a contiguous float32 tensor on {dev}")
            if inner and (n_rows - 1) * stride + inner > t.numel():
                raise ValueError(f"tensor {i}: {n_rows} rows of stride {stride} and {inner} elements do not fit {name}'s {t.numel()} elements")
        a.tensors[i] = _lib.SpdmObsNoiseTensor(d_src=src.data_ptr(), d_dst=dst.data_ptr(), inner=inner, src_stride=src_stride,
                                               dst_stride=dst_stride)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().spdm_obs_noise(index, ctypes.byref(a), stream), "spdm_obs_noise")


def perturb_observations(batch: dict, alpha: float, *, obs_horizon: int, seed: int = 0, draw: int = 0, row_offset: int = 0) -> dict:
    """A new dict with ``image``, ``position``, ``velocity`` and ``action`` of ``batch`` (a ``DeviceDataset.batch`` dict: float32
    device tensors ``(B, n, ...)`` with ``n >= obs_horizon``) cut to their first ``obs_horizon`` rows and perturbed:
    ``out[k] = batch[k][:, :obs_horizon] + alpha * u`` with ``u`` uniform in [0, 1), in one ``spdm_obs_noise`` launch on torch's
    current stream.  ``batch`` itself is not written.  Window ``b`` of the batch draws the stream of row ``row_offset + b``,
    ``draw`` selects an independent set of streams (``evaluation.robustness`` passes the noise level's number)."""
    obs_h = int(obs_horizon)
    if obs_h < 1:
        raise ValueError(f"obs_horizon = {obs_h} must be >= 1")
    missing = [k for k in OBSERVATION_KEYS if k not in batch]
    if missing:
        raise KeyError(f"batch holds no {missing}")
    B = batch[OBSERVATION_KEYS[0]].shape[0]
    out, tensors = {}, []
    for k in OBSERVATION_KEYS:
        t = batch[k]
        if t.dim() < 3 or t.shape[0] != B or t.shape[1] < obs_h:
            raise ValueError(f"batch[{k!r}] is {tuple(t.shape)}: expected {B} windows of at least {obs_h} rows")
        per_row = math.prod(t.shape[2:])
        out[k] = torch.empty((B, obs_h) + tuple(t.shape[2:]), dtype=torch.float32, device=t.device)
        tensors.append((t, out[k], obs_h * per_row, t.shape[1] * per_row, obs_h * per_row))
    add_uniform_noise(tensors, alpha, n_rows=B, seed=seed, draw=draw, row_offset=row_offset)
    return out


__all__ = ["forward_process", "add_uniform_noise", "perturb_observations", "OBSERVATION_KEYS"]
