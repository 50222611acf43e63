"""Gradient clipping + Adam on the device: ``DeviceAdam`` steps flat device parameters through ``spdm_adam_step``
(csrc/optim.hip) instead of ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam.step()``.

It stands where the reference's ``configure_optimizers`` (models/diffusion_ddpm.py:114-124,
models/encoder/autoencoder.py:73-74) puts ``torch.optim.Adam`` and where train.py's ``gradient_clip_val=0.5`` clips:
``Diffusion_DDPM.configure_optimizers(device_optimizer=True)`` and ``autoencoder.configure_optimizers(device_optimizer=True)``
build it.  A ``torch.optim.Optimizer`` subclass, so ``ReduceLROnPlateau`` drives ``param_groups[0]['lr']`` as it does Adam's,
and its state -- ``{'step', 'exp_avg', 'exp_avg_sq'}`` per parameter, torch tensors shaped and named as Adam's -- goes through
the base class's ``state_dict()`` / ``load_state_dict()`` in both directions between the two optimisers.

One difference from ``clip_grad_norm_``: ``.grad`` is only read; the clipped gradient exists inside the kernel alone.

``DeviceEMA`` keeps an exponential moving average of the same flat parameters through ``spdm_ema_step`` (one launch, the same
file) with ``ema_decay``'s warm-up schedule; ``Diffusion_DDPM.configure_ema`` builds it.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib

MAX_SEGMENTS = 4


def _adam_defaults(lr, betas, eps, weight_decay, amsgrad, maximize) -> dict:
    """The param-group keys of this torch's own Adam (so a state dict of either loads into the other), with our values."""
    probe = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps)
    d = dict(probe.defaults)
    d.update(weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
    return d


def _check_group(group) -> None:
    if group.get("weight_decay", 0) != 0:
        raise ValueError("DeviceAdam has no weight decay (weight_decay must be 0)")
    if group.get("amsgrad", False):
        raise ValueError("DeviceAdam has no amsgrad variant")
    if group.get("maximize", False):
        raise ValueError("DeviceAdam minimises (maximize must be False)")


def _check_flat_params(ps, who: str) -> None:
    """What DeviceAdam and DeviceEMA ask of their parameters: 1-4 flat segments for one launch."""
    if not 1 <= len(ps) <= MAX_SEGMENTS:
        raise ValueError(f"{who} takes 1 to {MAX_SEGMENTS} parameters, got {len(ps)}")
    for p in ps:
        if p.dim() != 1 or p.dtype != torch.float32 or not p.is_contiguous() or p.device.type != "cuda" or p.numel() == 0:
            raise ValueError(f"{who} parameters are flat, contiguous, non-empty fp32 tensors on the GPU "
                             f"(got shape {tuple(p.shape)}, {p.dtype}, {p.device})")
        if p.device != ps[0].device:
            raise ValueError(f"{who} parameters live on one device")


class DeviceAdam(torch.optim.Optimizer):
    """Adam (amsgrad=False, weight_decay=0) with optional global-norm clipping over 1-4 flat, contiguous fp32 device
    parameters, in one param group whose ``lr``, ``betas`` and ``eps`` are read at every step."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 amsgrad: bool = False, maximize: bool = False):
        defaults = _adam_defaults(lr, betas, eps, weight_decay, amsgrad, maximize)
        _check_group(defaults)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("DeviceAdam takes one param group")
        ps = self.param_groups[0]["params"]
        _check_flat_params(ps, "DeviceAdam")
        self._lib = _lib.load()
        self._device = ps[0].device
        self._device_index = self._device.index if self._device.index is not None else torch.cuda.current_device()
        self._norm_index = int(self._lib.spdm_adam_norm_index())
        self._workspace = torch.empty(int(self._lib.spdm_adam_workspace_doubles()), dtype=torch.float64, device=self._device)
        self._clipped = False

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:        # as torch.optim.Adam initialises it (step: a host scalar tensor)
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None, max_norm: Optional[float] = None):
        """One step on torch's current stream; nothing synchronises.  ``max_norm``: clip the global gradient norm over all
        parameters first (None / 0: no clipping)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        _check_group(group)
        beta1, beta2 = group["betas"]
        ps = group["params"]
        segs = (_lib.SpdmOptimSegment * len(ps))()
        steps = set()
        for i, p in enumerate(ps):
            if p.grad is None:
                raise RuntimeError(f"DeviceAdam.step: parameter {i} has no .grad")
            g = p.grad
            if g.is_sparse or g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                raise RuntimeError(f"DeviceAdam.step: parameter {i}'s .grad is not a contiguous fp32 tensor of its shape and device")
            st = self._state_of(p)
            for k in ("exp_avg", "exp_avg_sq"):
                m = st[k]
                if m.dtype != torch.float32 or m.device != p.device or m.shape != p.shape or not m.is_contiguous():
                    raise RuntimeError(f"DeviceAdam.step: state[{k!r}] of parameter {i} is not a contiguous fp32 tensor like it")
            steps.add(int(float(st["step"])))
            segs[i] = _lib.SpdmOptimSegment(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                            p.numel())
        if len(steps) != 1:
            raise RuntimeError(f"DeviceAdam.step: the parameters' step counts differ ({sorted(steps)}): one group steps together")
        step = steps.pop() + 1
        clip = float(max_norm) if max_norm else 0.0
        stream = ctypes.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)
        _lib.check(self._lib.spdm_adam_step(self._device_index, segs, len(ps), step, float(group["lr"]), float(beta1),
                                            float(beta2), float(group["eps"]), clip,
                                            ctypes.c_void_p(self._workspace.data_ptr()), stream), "spdm_adam_step")
        for p in ps:
            self.state[p]["step"] += 1
        self._clipped = clip > 0.0
        return loss

    @property
    def last_grad_norm(self) -> Optional[float]:
        """The global gradient norm the last step clipped by (float64, before clipping); None when that step did not clip.
        Reads the workspace: the one call here that synchronises."""
        if not self._clipped:
            return None
        return float(self._workspace[self._norm_index].item())


EMA_SCHEDULE = {"update_after_step": 0, "inv_gamma": 1.0, "power": 0.75, "min_value": 0.0, "max_value": 0.9999}


def ema_decay(step: int, *, update_after_step: int = 0, inv_gamma: float = 1.0, power: float = 0.75, min_value: float = 0.0,
              max_value: float = 0.9999) -> float:
    """The decay of EMA update number ``step`` (1 for the first): the warm-up schedule of diffusers' ``EMAModel`` as
    diffusion-policy uses it.  With ``n = max(0, step - update_after_step - 1)`` it is 0 for ``n == 0`` (the shadow takes the
    weights) and ``clamp(1 - (1 + n / inv_gamma) ** -power, min_value, max_value)`` otherwise, in Python floats.

    This restates the library from memory: it is pinned against no value computed by diffusers (8.19 says the
    same of the solver)."""
    n = max(0, int(step) - int(update_after_step) - 1)
    if n == 0:
        return 0.0
    value = 1.0 - (1.0 + n / float(inv_gamma)) ** -float(power)
    return max(float(min_value), min(value, float(max_value)))


class DeviceEMA:
    """An exponential moving average of 1-4 flat fp32 device parameters -- the optimiser's -- kept by ``spdm_ema_step``
    (csrc/optim.hip): ``shadow[i]`` follows ``params[i]`` as ``s.sub_((1 - decay) * (s - p))``, bit for bit what
    torch computes for that recipe, in one launch for all parameters.  The decay of each update comes from ``ema_decay`` with
    this object's schedule arguments.  The parameters are only read, so it works beside ``DeviceAdam`` and beside
    ``torch.optim.Adam`` alike; the state is plain torch tensors and an integer."""

    def __init__(self, params, **schedule):
        unknown = sorted(set(schedule) - set(EMA_SCHEDULE))
        if unknown:
            raise TypeError(f"DeviceEMA: unknown schedule argument(s) {unknown} (known: {sorted(EMA_SCHEDULE)})")
        self.params = list(params)
        _check_flat_params(self.params, "DeviceEMA")
        self.schedule = dict(EMA_SCHEDULE, **schedule)
        ema_decay(1, **self.schedule)                      # (a bad value raises here, not at the first step)
        self._lib = _lib.load()
        self._device = self.params[0].device
        self._device_index = self._device.index if self._device.index is not None else torch.cuda.current_device()
        with torch.no_grad():
            self.shadow = [torch.empty_like(p).copy_(p) for p in self.params]
        self.optimization_step = 0

    @torch.no_grad()
    def step(self) -> float:
        """One update of every shadow from its parameter's current values: ONE launch on torch's current stream; nothing
        synchronises.  Returns the decay used."""
        self.optimization_step += 1
        decay = ema_decay(self.optimization_step, **self.schedule)
        segs = (_lib.SpdmEmaSegment * len(self.params))()
        for i, (s, p) in enumerate(zip(self.shadow, self.params)):
            if s.shape != p.shape or s.dtype != torch.float32 or s.device != p.device or not s.is_contiguous():
                raise RuntimeError(f"DeviceEMA.step: shadow {i} is not a contiguous fp32 tensor like its parameter")
            segs[i] = _lib.SpdmEmaSegment(s.data_ptr(), p.data_ptr(), p.numel())
        stream = ctypes.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)
        _lib.check(self._lib.spdm_ema_step(self._device_index, segs, len(segs), 1.0 - decay, stream), "spdm_ema_step")
        return decay

    def state_dict(self) -> dict:
        """``{'shadow': [tensor, ...], 'optimization_step': int, 'schedule': {...}}`` (the tensors are the live ones)."""
        return {"shadow": list(self.shadow), "optimization_step": int(self.optimization_step), "schedule": dict(self.schedule)}

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        """Take the counter and copy the shadow tensors in; raises if the schedule differs from this object's or the shadow
        does not fit the parameters."""
        sched = dict(state["schedule"])
        if sched != self.schedule:
            raise ValueError(f"DeviceEMA.load_state_dict: the state's schedule {sched} is not this EMA's {self.schedule}")
        shadow = list(state["shadow"])
        if len(shadow) != len(self.shadow) or any(tuple(a.shape) != tuple(b.shape) for a, b in zip(shadow, self.shadow)):
            raise ValueError("DeviceEMA.load_state_dict: the state's shadow tensors do not match the parameters")
        for mine, theirs in zip(self.shadow, shadow):
            mine.copy_(theirs.to(torch.float32))
        self.optimization_step = int(state["optimization_step"])


__all__ = ["DeviceAdam", "DeviceEMA", "EMA_SCHEDULE", "MAX_SEGMENTS", "ema_decay"]
