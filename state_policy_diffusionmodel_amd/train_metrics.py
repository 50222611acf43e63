"""The loss of a validation pass on the device: ``loss_terms_into`` is one ``spdm_loss_terms`` launch
(csrc/train_metrics.hip) that turns a batch's predicted and drawn noise into per-sample mean squared errors at the batch's
slots of a pass-wide float64 buffer; ``evaluation.reduce_errors`` over that buffer gives the pass's mean.
``recon_terms_into`` is the same for the frame autoencoder (``spdm_recon_terms``): a batch's frames and their
reconstructions into per-frame mean squared errors.

There is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib


def loss_terms_into(eps: torch.Tensor, noise: torch.Tensor, terms: torch.Tensor, slot_offset: int = 0, *,
                    t: Optional[torch.Tensor] = None, slot_t: Optional[torch.Tensor] = None) -> None:
    """``terms[slot_offset + b] = mean(((double)noise[b] - (double)eps[b]) ** 2)`` for the B samples of ``eps`` / ``noise``
    ((B, H, D) or (B, 1, H, D) contiguous fp32 device tensors), on torch's current stream; ``terms`` is a contiguous float64
    device vector.  ``t`` (B, int32) with ``slot_t`` (int32, ``terms``' length), both or neither: ``slot_t[slot_offset + b] =
    t[b]``.  Slots outside ``[slot_offset, slot_offset + B)`` are not touched."""
    if eps.shape != noise.shape or eps.dim() not in (3, 4) or (eps.dim() == 4 and eps.shape[1] != 1):
        raise ValueError(f"eps and noise must both be (B,H,D) or (B,1,H,D), got {tuple(eps.shape)} and {tuple(noise.shape)}")
    for name, v, dt in (("eps", eps, torch.float32), ("noise", noise, torch.float32), ("terms", terms, torch.float64),
                        ("t", t, torch.int32), ("slot_t", slot_t, torch.int32)):
        if v is not None and (not v.is_cuda or v.dtype != dt or not v.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dt} device tensor")
    B, H, D = eps.shape[0], eps.shape[-2], eps.shape[-1]
    if terms.dim() != 1 or (slot_t is not None and slot_t.shape != terms.shape) or (t is not None and t.numel() != B):
        raise ValueError("terms must be a vector, slot_t of its length, t of B elements")
    p = lambda v: v.data_ptr() if v is not None else None  # noqa: E731
    a = _lib.SpdmLossTermsArgs(B=B, H=H, D=D, reserved=0, d_eps=p(eps), d_noise=p(noise), slot_offset=int(slot_offset),
                               n_slots=terms.numel(), d_terms=p(terms), d_t_in=p(t), d_slot_t=p(slot_t))
    stream = ctypes.c_void_p(torch.cuda.current_stream(eps.device).cuda_stream)
    _lib.check(_lib.load().spdm_loss_terms(eps.device.index, ctypes.byref(a), stream), "spdm_loss_terms")


def recon_terms_into(recon: torch.Tensor, target: torch.Tensor, terms: torch.Tensor, slot_offset: int = 0) -> None:
    """``terms[slot_offset + b] = mean(((double)target[b] - (double)recon[b]) ** 2)`` for the n frames of ``recon`` /
    ``target`` ((n,3,96,96) contiguous fp32 device tensors), ONE ``spdm_recon_terms`` launch on torch's current stream
    (DESIGN.md 8.23); ``terms`` is a contiguous float64 device vector.  Slots outside ``[slot_offset, slot_offset + n)``
    are not touched."""
    if recon.shape != target.shape or recon.dim() != 4 or tuple(recon.shape[1:]) != (3, 96, 96):
        raise ValueError(f"recon and target must both be (n,3,96,96), got {tuple(recon.shape)} and {tuple(target.shape)}")
    for name, v, dt in (("recon", recon, torch.float32), ("target", target, torch.float32), ("terms", terms, torch.float64)):
        if not v.is_cuda or v.dtype != dt or not v.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} device tensor")
    if terms.dim() != 1:
        raise ValueError("terms must be a vector")
    a = _lib.SpdmReconTermsArgs(n=recon.shape[0], reserved=0, d_recon=recon.data_ptr(), d_target=target.data_ptr(),
                                slot_offset=int(slot_offset), n_slots=terms.numel(), d_terms=terms.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(recon.device).cuda_stream)
    _lib.check(_lib.load().spdm_recon_terms(recon.device.index, ctypes.byref(a), stream), "spdm_recon_terms")


__all__ = ["loss_terms_into", "recon_terms_into"]
