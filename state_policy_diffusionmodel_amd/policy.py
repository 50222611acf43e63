"""The closed-loop caller of ``sample()`` with its host side on the device.

Replaces run_predictions.py:30-60 and :112-168 around the ``sample`` call: the four ``deque(maxlen=obs_horizon * step_size)``,
``prepare_diffusion_batch`` (``torch.tensor(list(deque)[::s])`` over every 96x96x3 frame of the window on every environment
step, float32 normalisation on the CPU, a host-to-device copy of the whole window per call) and the ``.cpu()`` + numpy
``unnormalize_position`` on the way out.  ``ClosedLoopPolicy`` keeps the history of E environments in HBM as rings
(``spdm_policy_push``: one launch per step), builds the conditioning batch in one launch (``spdm_policy_window``), samples
with the model's engine and returns way-points and actions in the dataset's units from one more launch
(``spdm_policy_unnormalize``).  E = 1 is the reference's loop; a larger E drives that many environments in lockstep.

There is no CPU fallback: every method but the constructor's checks needs the GPU."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

FRAME_SHAPE = (96, 96, 3)


@dataclass
class Plan:
    """Device tensors: ``waypoints`` (E, pred_horizon, 2) float64 positions in the dataset's units, ``actions``
    (E, pred_horizon, 3) float64 or None (a model whose prediction_dim holds no action), ``x_0`` (E, 1, H, D) float32 as the
    sampler returned it."""
    waypoints: torch.Tensor
    actions: Optional[torch.Tensor]
    x_0: torch.Tensor


def _channel_stats(stats: dict, key: str, n: int):
    """``(min, max, is_float32)`` of ``stats[key]``: float64 lists of ``n`` channels, and whether the ARRAYS are float32 --
    torch promotes ``tensor - array`` by the array's dtype, so the reference's arithmetic depends on it."""
    lo, hi = np.asarray(stats[key]["min"]), np.asarray(stats[key]["max"])
    if lo.dtype != hi.dtype or lo.dtype not in (np.float32, np.float64):
        raise ValueError(f"stats[{key!r}]: min and max must both be float32 or both float64 arrays, got {lo.dtype} and {hi.dtype}")
    if lo.reshape(-1).shape != (n,) or hi.reshape(-1).shape != (n,):
        raise ValueError(f"stats[{key!r}] must have {n} channels, got {lo.shape} and {hi.shape}")
    return lo.reshape(-1).astype(np.float64).tolist(), hi.reshape(-1).astype(np.float64).tolist(), lo.dtype == np.float32


class ClosedLoopPolicy:
    """``model``: a ``Diffusion_DDPM`` / ``Diffusion_DDIM``; ``stats``: the training run's statistics dict; ``n_envs``:
    environments driven in lockstep; ``image_storage``: ``'uint8'`` (raw pixels, divided by 255 when the batch is built) or
    ``'float32'`` (values the model takes as they are).  ``obs_horizon``, ``pred_horizon`` and ``inpaint_horizon`` are the
    model's; ``step_size`` is the model's (its hparams') unless given.  A new policy has every environment pending a fill."""

    def __init__(self, model, stats: dict, n_envs: int = 1, image_storage: str = "uint8", device: int = 0,
                 step_size: Optional[int] = None):
        if image_storage not in ("uint8", "float32"):
            raise ValueError(f"image_storage must be 'uint8' or 'float32', got {image_storage!r}")
        self.model, self.stats, self.n_envs, self.image_storage = model, stats, int(n_envs), image_storage
        self.obs_horizon, self.pred_horizon = int(model.obs_horizon), int(model.pred_horizon)
        self.inpaint_horizon, self.prediction_dim = int(model.inpaint_horizon), int(model.prediction_dim)
        self.step_size = int(model.step_size if step_size is None else step_size)
        self.device = torch.device("cuda", device)
        if self.n_envs < 1 or self.step_size < 1 or self.obs_horizon < 1 or self.pred_horizon < 1:
            raise ValueError(f"n_envs = {self.n_envs}, step_size = {self.step_size}, obs_horizon = {self.obs_horizon} and "
                             f"pred_horizon = {self.pred_horizon} must all be >= 1")
        if model.device != self.device:
            raise ValueError(f"policy on {self.device}, model on {model.device}")
        if self.prediction_dim < 2:
            raise ValueError(f"prediction_dim = {self.prediction_dim} holds no position")
        self._pos_min, self._pos_max = float(stats["position"]["min"]), float(stats["position"]["max"])
        self._vel_min, self._vel_max, vel_f32 = _channel_stats(stats, "velocity", 2)
        self._act_min, self._act_max, act_f32 = _channel_stats(stats, "action", 3)
        self._stats_f32 = int(vel_f32) | int(act_f32) << 1
        self.history = self.obs_horizon * self.step_size                      # L: slots per environment
        E, L, dev = self.n_envs, self.history, self.device
        self._img_dtype = torch.uint8 if image_storage == "uint8" else torch.float32
        self._ring_img = torch.empty((E, L) + FRAME_SHAPE, dtype=self._img_dtype, device=dev)
        self._ring_pos = torch.empty((E, L, 2), dtype=torch.float32, device=dev)
        self._ring_vel = torch.empty((E, L, 2), dtype=torch.float32, device=dev)
        self._ring_act = torch.empty((E, L, 3), dtype=torch.float32, device=dev)
        self._fill = torch.ones(E, dtype=torch.int32, device=dev)
        self._fill_set = True                                                  # some entry of _fill is non-zero
        self.pushes = 0                                                        # n: observations taken so far

    # ---- history --------------------------------------------------------------------------------------------------------------
    def reset(self, env_ids=None) -> None:
        """The next ``observe()`` fills the whole history of the environments ``env_ids`` (all by default) with their
        observation, as run_predictions.py:120-124 does before its loop."""
        if env_ids is None:
            self._fill.fill_(1)
        else:
            ids = np.asarray(env_ids).reshape(-1)
            if ids.size and (not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= self.n_envs):
                raise IndexError(f"env_ids must be integers in [0, {self.n_envs}), got {ids.tolist()}")
            if ids.size == 0:
                return
            self._fill[torch.from_numpy(ids.astype(np.int64)).to(self.device)] = 1
        self._fill_set = True

    def _input(self, name: str, x, shape, dtype) -> torch.Tensor:
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
        if dtype is None:                                                      # low-dimensional: rounded to float32 on entry
            if not (t.dtype.is_floating_point or t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
                raise TypeError(f"{name} must be a real-valued array, got {t.dtype}")
            dtype = torch.float32
        elif t.dtype != dtype:
            raise TypeError(f"{name} must be {dtype} (image_storage={self.image_storage!r}), got {t.dtype}")
        return t.to(device=self.device, dtype=dtype).contiguous()

    def observe(self, img, position, velocity, action) -> None:
        """One observation per environment -- ``img`` (E,96,96,3) in the storage's dtype, ``position`` (E,2), ``velocity``
        (E,2), ``action`` (E,3), host or device -- into the history, in ONE launch on torch's current stream."""
        E, L = self.n_envs, self.history
        img = self._input("img", img, (E,) + FRAME_SHAPE, self._img_dtype)
        pos = self._input("position", position, (E, 2), None)
        vel = self._input("velocity", velocity, (E, 2), None)
        act = self._input("action", action, (E, 3), None)
        a = _lib.SpdmPolicyPushArgs(E=E, L=L, img_dtype=0 if self.image_storage == "uint8" else 1, reserved=0, n=self.pushes,
                                    d_img_in=img.data_ptr(), d_pos_in=pos.data_ptr(), d_vel_in=vel.data_ptr(), d_act_in=act.data_ptr(),
                                    d_fill=self._fill.data_ptr(), d_ring_img=self._ring_img.data_ptr(),
                                    d_ring_pos=self._ring_pos.data_ptr(), d_ring_vel=self._ring_vel.data_ptr(),
                                    d_ring_act=self._ring_act.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().spdm_policy_push(self.device.index, ctypes.byref(a), stream), "spdm_policy_push")
        if self._fill_set:
            self._fill.zero_()
            self._fill_set = False
        self.pushes += 1

    # ---- the conditioning batch -----------------------------------------------------------------------------------------------
    def batch(self) -> dict:
        """``{'image' (E,obs_h,3,96,96), 'position' (E,obs_h,2), 'velocity' (E,obs_h,2), 'action' (E,obs_h,3), 'translation'
        (E,2)}``: float32 device tensors, what ``prepare_diffusion_batch`` builds from ``list(deque)[::step_size]``, in ONE
        launch on torch's current stream."""
        if self.pushes < 1:
            raise RuntimeError("ClosedLoopPolicy.batch() before the first observe(): the history is empty")
        E, obs_h, dev = self.n_envs, self.obs_horizon, self.device
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        out = {"image": f32(E, obs_h, 3, 96, 96), "position": f32(E, obs_h, 2), "velocity": f32(E, obs_h, 2),
               "action": f32(E, obs_h, 3), "translation": f32(E, 2)}
        a = _lib.SpdmPolicyWindowArgs(E=E, L=self.history, obs_h=obs_h, step_size=self.step_size,
                                      img_dtype=0 if self.image_storage == "uint8" else 1, stats_f32=self._stats_f32, n=self.pushes,
                                      d_ring_img=self._ring_img.data_ptr(), d_ring_pos=self._ring_pos.data_ptr(),
                                      d_ring_vel=self._ring_vel.data_ptr(), d_ring_act=self._ring_act.data_ptr(),
                                      pos_min=self._pos_min, pos_max=self._pos_max,
                                      d_image_out=out["image"].data_ptr(), d_position_out=out["position"].data_ptr(),
                                      d_velocity_out=out["velocity"].data_ptr(), d_action_out=out["action"].data_ptr(),
                                      d_translation_out=out["translation"].data_ptr())
        a.vel_min[:], a.vel_max[:], a.act_min[:], a.act_max[:] = self._vel_min, self._vel_max, self._act_min, self._act_max
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().spdm_policy_window(dev.index, ctypes.byref(a), stream), "spdm_policy_window")
        return out

    # ---- the plan -------------------------------------------------------------------------------------------------------------
    def unnormalize(self, x_0: torch.Tensor, translation: torch.Tensor) -> Plan:
        """``x_0`` (E,1,H,D) or (E,H,D) float32 and ``translation`` (E,2) float32, device tensors, as a ``Plan``: ONE launch."""
        x = x_0[:, 0] if x_0.dim() == 4 else x_0
        for name, t in (("x_0", x), ("translation", translation)):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous float32 device tensor")
        E, H, D = x.shape
        P = H - self.inpaint_horizon
        if E != self.n_envs or P < 1 or D < 2 or tuple(translation.shape) != (E, 2):
            raise ValueError(f"x_0 must be ({self.n_envs}, H > {self.inpaint_horizon}, D >= 2) and translation ({self.n_envs}, 2); got "
                             f"{tuple(x.shape)} and {tuple(translation.shape)}")
        way = torch.empty((E, P, 2), dtype=torch.float64, device=self.device)
        act = torch.empty((E, P, 3), dtype=torch.float64, device=self.device) if D >= 5 else None
        a = _lib.SpdmPolicyUnnormalizeArgs(E=E, H=H, D=D, inp_h=self.inpaint_horizon, d_x0=x.data_ptr(), d_translation=translation.data_ptr(),
                                           pos_min=self._pos_min, pos_max=self._pos_max, d_waypoints=way.data_ptr(),
                                           d_actions=act.data_ptr() if act is not None else None)
        a.act_min[:], a.act_max[:] = self._act_min, self._act_max
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().spdm_policy_unnormalize(self.device.index, ctypes.byref(a), stream), "spdm_policy_unnormalize")
        return Plan(waypoints=way, actions=act, x_0=x_0)

    def plan(self, seed: Optional[int] = None, x_T: Optional[torch.Tensor] = None) -> Plan:
        """``batch()``, ``model.sample(batch, batched=True, sharded=False, seed=seed, x_T=x_T)`` and one unnormalise launch.
        Nothing is copied to the host.  ``seed`` and ``x_T`` are ``sample``'s: left at None they are drawn per call."""
        batch = self.batch()
        x_0 = self.model.sample(dict(batch), batched=True, sharded=False, seed=seed, x_T=x_T)
        return self.unnormalize(x_0.contiguous(), batch["translation"])


__all__ = ["ClosedLoopPolicy", "Plan"]
