"""The closed-loop caller of ``sample()`` with its host side on the device.

Replaces run_predictions.py:30-60 and :112-168 around the ``sample`` call: the four ``deque(maxlen=obs_horizon * step_size)``,
``prepare_diffusion_batch`` (``torch.tensor(list(deque)[::s])`` over every 96x96x3 frame of the window on every environment
step, float32 normalisation on the CPU, a host-to-device copy of the whole window per call) and the ``.cpu()`` + numpy
``unnormalize_position`` on the way out.  ``ClosedLoopPolicy`` keeps the history of E environments in HBM as rings
(``spdm_policy_push``: one launch per step), builds the conditioning batch in one launch (``spdm_policy_window``), samples
with the model's engine and returns way-points and actions in the dataset's units from one more launch
(``spdm_policy_unnormalize``).  E = 1 is the reference's loop; a larger E drives that many environments in lockstep.
``plan(warm_start=K)`` replans from the previous plan instead of from noise: one more launch
(``spdm_policy_warm_start``) shifts, re-centres and re-noises it, and only the last K denoise steps run.
``plan_candidates(candidates=K)`` samples K candidates per environment and keeps one, chosen on the device: one more
launch (``spdm_policy_select``) scores them against the plan being executed, or against each other, and reports their spread.

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
    sampler returned it.  ``steps``: denoise iterations ``plan()`` ran for it (0: not made by ``plan()``); ``warm``: whether
    it started from the previous plan."""
    waypoints: torch.Tensor
    actions: Optional[torch.Tensor]
    x_0: torch.Tensor
    steps: int = 0
    warm: bool = False


@dataclass
class CandidatePlan(Plan):
    """What ``plan_candidates()`` returns: a ``Plan`` whose ``x_0``, ``waypoints`` and ``actions`` are the chosen candidate's.
    ``candidates``: trajectories sampled per environment.  With ``candidates > 1`` (None otherwise): ``selected_by`` what chose
    among them (``'coherent'``, ``'medoid'`` or ``'first'``), ``chosen`` (E) int32 the index kept, ``scores`` (E, K) float64 the
    candidates' scores and ``spread`` (E, pred_horizon) float64 the RMS distance of the candidates' way-points from their mean,
    in the dataset's units: device tensors."""
    candidates: int = 1
    selected_by: str = ''
    chosen: Optional[torch.Tensor] = None
    scores: Optional[torch.Tensor] = None
    spread: Optional[torch.Tensor] = None


SELECT_MODES = ("coherent", "medoid", "first")
MAX_CANDIDATES = 64


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
        # the previous plan, for plan(warm_start=K): x_0 and translation stay on the device
        self._prev_x0: Optional[torch.Tensor] = None
        self._prev_translation: Optional[torch.Tensor] = None
        self._prev_pushes = 0                                                  # the push count it was made at
        self._prev_usable = False                                              # False again after any reset()
        self.plans = 0                                                         # plan() calls so far: the warm start's `draw`
        self._levels = (None, None, None)                                      # (scheduler object, noise_steps, its (n, 6) table)
        # how the last plan_candidates(candidates > 1) scored its candidates: {'scored_by': 'coherent' | 'medoid', 'rows', 'cols'}
        self.last_selection: Optional[dict] = None

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
        self._prev_usable = False                                              # lockstep: one loop serves all, so all plan cold

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

    def warm_start(self, prev_x0: torch.Tensor, prev_translation: torch.Tensor, translation: torch.Tensor,
                   inpaint: Optional[torch.Tensor], delta: int, sa: float, sb: float, seed: int, draw: int, *, env_offset: int = 0,
                   noise: Optional[torch.Tensor] = None, return_parts: bool = False):
        """The starting iterate (E,1,H,D) of a loop suffix from the plan ``prev_x0`` (E,1,H,D) or (E,H,D) made ``delta``
        pushes ago: ONE launch (``spdm_policy_warm_start``, include/spdm.h) on torch's current stream.  ``inpaint``
        (E,inp_h,D) or None when the model in-paints nothing; ``noise`` (E,H,D): the caller's instead of the drawn one.
        ``return_parts=True``: ``(x, guess, noise)``, the shifted plan before noising and the noise used as well."""
        x0 = prev_x0[:, 0] if prev_x0.dim() == 4 else prev_x0
        E, H, D = x0.shape
        inp_h = self.inpaint_horizon
        given = [("prev_x0", x0, (E, H, D)), ("prev_translation", prev_translation, (E, 2)), ("translation", translation, (E, 2))]
        if inp_h > 0:
            if inpaint is None:
                raise ValueError(f"inpaint is None with inpaint_horizon = {inp_h}")
            given.append(("inpaint", inpaint, (E, inp_h, D)))
        if noise is not None:
            given.append(("noise", noise, (E, H, D)))
        for name, t, shape in given:
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"{name} must be a contiguous float32 device tensor of shape {shape}, got {tuple(t.shape)} {t.dtype}")
        x = torch.empty((E, 1, H, D), dtype=torch.float32, device=self.device)
        guess = torch.empty((E, H, D), dtype=torch.float32, device=self.device) if return_parts else None
        used = noise if noise is not None or not return_parts else torch.empty((E, H, D), dtype=torch.float32, device=self.device)
        a = _lib.SpdmPolicyWarmStartArgs(E=E, H=H, D=D, inp_h=inp_h, step_size=self.step_size, draw=int(draw) & 0xFFFFFFFF,
                                         delta=int(delta), seed=int(seed), env_offset=int(env_offset), sa=float(sa), sb=float(sb),
                                         d_prev_x0=x0.data_ptr(), d_prev_translation=prev_translation.data_ptr(),
                                         d_translation=translation.data_ptr(), d_inpaint=inpaint.data_ptr() if inp_h > 0 else None,
                                         d_noise_in=noise.data_ptr() if noise is not None else None, d_x=x.data_ptr(),
                                         d_guess=guess.data_ptr() if guess is not None else None,
                                         d_noise=used.data_ptr() if return_parts else None)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().spdm_policy_warm_start(self.device.index, ctypes.byref(a), stream), "spdm_policy_warm_start")
        return (x, guess, used) if return_parts else x

    def select(self, x_0: torch.Tensor, candidates: int, mode: str = "medoid", *, guess: Optional[torch.Tensor] = None, rows: int = 0,
               guess_row_stride: int = 1, cols: int = 2, translation: Optional[torch.Tensor] = None):
        """One of ``candidates`` = K plans per environment: ONE launch (``spdm_policy_select``, include/spdm.h) on torch's
        current stream.  ``x_0`` (E K,1,H,D) or (E K,H,D) float32, candidate k of environment e in row e K + k; ``mode``
        ``'medoid'`` or ``'coherent'``, the latter against ``guess`` (rows of (H,D), environment e's at row e
        ``guess_row_stride``) over its first ``rows`` predicted rows; ``cols`` columns enter a distance; ``translation`` (E,2)
        asks for the spread.  Returns ``(chosen (E) int32, x_0 (E,1,H,D) float32, scores (E,K) float64, spread (E,P) float64
        or None)``, device tensors."""
        if mode not in ("medoid", "coherent"):
            raise ValueError(f"mode must be 'medoid' or 'coherent', got {mode!r}")
        x = x_0[:, 0] if x_0.dim() == 4 else x_0
        K, E = int(candidates), self.n_envs
        if x.dim() != 3:
            raise ValueError(f"x_0 must be (E K, 1, H, D) or (E K, H, D), got {tuple(x_0.shape)}")
        given = [("x_0", x, (E * K,) + tuple(x.shape[1:]))]
        if translation is not None:
            given.append(("translation", translation, (E, 2)))
        if guess is not None:
            given.append(("guess", guess, tuple(guess.shape[:1]) + tuple(x.shape[1:])))
        for name, t, shape in given:
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"{name} must be a contiguous float32 device tensor of shape {shape}, got {tuple(t.shape)} {t.dtype}")
        if guess is not None and guess_row_stride >= 1 and guess.shape[0] < (E - 1) * guess_row_stride + 1:
            raise ValueError(f"guess has {guess.shape[0]} rows: environment {E - 1} reads row {(E - 1) * guess_row_stride}")
        _, H, D = x.shape
        P = H - self.inpaint_horizon
        dev = self.device
        chosen = torch.empty(E, dtype=torch.int32, device=dev)
        out = torch.empty((E, 1, H, D), dtype=torch.float32, device=dev)
        scores = torch.empty((E, K), dtype=torch.float64, device=dev)
        spread = torch.empty((E, max(P, 0)), dtype=torch.float64, device=dev) if translation is not None else None
        a = _lib.SpdmPolicySelectArgs(E=E, K=K, H=H, D=D, inp_h=self.inpaint_horizon, cols=int(cols),
                                      mode=_lib.SPDM_SELECT_COHERENT if mode == "coherent" else _lib.SPDM_SELECT_MEDOID,
                                      rows=int(rows), guess_row_stride=int(guess_row_stride), d_x0=x.data_ptr(),
                                      d_guess=guess.data_ptr() if guess is not None else None,
                                      d_translation=translation.data_ptr() if translation is not None else None,
                                      pos_min=self._pos_min, pos_max=self._pos_max, d_chosen=chosen.data_ptr(), d_x0_out=out.data_ptr(),
                                      d_scores=scores.data_ptr(), d_spread=spread.data_ptr() if spread is not None else None)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().spdm_policy_select(dev.index, ctypes.byref(a), stream), "spdm_policy_select")
        return chosen, out, scores, spread

    def _noise_level(self, i0: int):
        """``(sa, sb)`` = (sqrt(abar_t), sqrt(1 - abar_t)) of the timestep loop iteration ``i0`` denoises from: row ``i0`` of the
        table ``sample()`` installs in the engine, the same float32 values."""
        from .diffusion import _as_spec
        sched, N = self.model.noise_scheduler, int(self.model.noise_steps)
        if self._levels[0] is not sched or self._levels[1] != N:
            spec = _as_spec(sched)
            spec.set_timesteps(N)
            self._levels = (sched, N, np.ascontiguousarray(spec.coefficient_table(), dtype=np.float32))
        row = self._levels[2][i0]
        return float(row[1]), float(row[0])

    def plan(self, seed: Optional[int] = None, x_T: Optional[torch.Tensor] = None, warm_start: Optional[int] = None) -> Plan:
        """``batch()``, ``model.sample(batch, batched=True, sharded=False, seed=seed, x_T=x_T)`` and one unnormalise launch.
        Nothing is copied to the host.  ``seed`` and ``x_T`` are ``sample``'s: left at None they are drawn per call.

        ``warm_start = K`` (1 <= K <= the model's ``noise_steps`` N; ValueError otherwise) asks for the last K iterations of
        the loop only.  The plan is WARM when there is a previous plan, no ``reset()`` came since (the environments run in
        lockstep, so one loop serves all) and at most ``(pred_horizon - 1) step_size`` observations did: one
        ``spdm_policy_warm_start`` launch shifts the previous ``x_0`` by the observations since, re-centres it on the new
        window and noises it to the level iteration N - K starts from, and ``model.sample(..., start_step=N - K)`` runs the
        rest.  A warm plan ignores ``x_T``.  Otherwise the plan is COLD: exactly the path above, all N iterations.
        ``Plan.steps`` and ``Plan.warm`` say which it was."""
        return self._plan(seed, x_T, warm_start, 1, "coherent", 2)[0]

    def plan_candidates(self, seed: Optional[int] = None, x_T: Optional[torch.Tensor] = None, warm_start: Optional[int] = None,
                        candidates: int = 1, select: str = "coherent", cols: int = 2) -> CandidatePlan:
        """``plan()`` from ``candidates = K`` (1 <= K <= 64) trajectories per environment, one of which is kept:
        ``sample(..., candidates=K)`` builds and encodes the batch once per environment (``x_T``, if given, is (E K,1,H,D)), ONE
        ``spdm_policy_select`` launch chooses, and the way-points, the actions, ``x_0`` and the plan the next warm start or
        selection refers to are the chosen candidate's.  Nothing is copied to the host.  ``select='coherent'`` keeps the
        candidate closest to the previous chosen plan, shifted and re-centred as a warm start does, over the rows that plan
        still informs -- when a previous plan is usable, which is ``plan()``'s condition for a warm plan; otherwise, and with
        ``select='medoid'``, the candidate with the smallest sum of squared distances to the others.  ``select='first'`` keeps
        candidate 0 whatever the scores say (for A/B runs); scores and spread are still those ``'coherent'`` would have
        reported.  ``cols``: the columns that enter a distance, 2 (positions) to ``prediction_dim`` (positions and actions).
        With ``warm_start`` the warm iterate is built for all E K rows, each with noise of its own.  ``candidates = 1`` makes
        exactly the calls of ``plan()``: no select launch, and the selection's fields stay None.  ``plan()`` and
        ``plan_candidates()`` share the policy's state and may alternate."""
        if isinstance(candidates, bool) or not isinstance(candidates, (int, np.integer)) or not 1 <= candidates <= MAX_CANDIDATES:
            raise ValueError(f"candidates = {candidates!r} must be an integer in [1, {MAX_CANDIDATES}]")
        if select not in SELECT_MODES:
            raise ValueError(f"select = {select!r} must be one of {SELECT_MODES}")
        if isinstance(cols, bool) or not isinstance(cols, (int, np.integer)) or not 2 <= cols <= self.prediction_dim:
            raise ValueError(f"cols = {cols!r} must be an integer in [2, prediction_dim = {self.prediction_dim}]")
        plan, picked = self._plan(seed, x_T, warm_start, int(candidates), select, int(cols))
        return CandidatePlan(waypoints=plan.waypoints, actions=plan.actions, x_0=plan.x_0, steps=plan.steps, warm=plan.warm, **picked)

    def _plan(self, seed, x_T, warm_start, K: int, select: str, cols: int):
        """``(Plan, the selection's fields)`` of ``plan()`` (K = 1) and ``plan_candidates()``, arguments validated but ``warm_start``."""
        if warm_start is not None:
            N = int(self.model.noise_steps)
            if isinstance(warm_start, bool) or not isinstance(warm_start, (int, np.integer)) or not 1 <= warm_start <= N:
                raise ValueError(f"warm_start = {warm_start!r} must be an integer in [1, noise_steps = {N}]")
        H, D = self.pred_horizon + self.inpaint_horizon, self.prediction_dim
        if K > 1 and x_T is not None and tuple(x_T.shape) != (self.n_envs * K, 1, H, D):
            raise ValueError(f"x_T must be {(self.n_envs * K, 1, H, D)} with candidates = {K}, got {tuple(x_T.shape)}")
        batch = self.batch()
        N = int(self.model.noise_steps)
        if seed is None:                                                       # sample()'s recipe, drawn here so that the warm
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())      # start and the loop share one seed
        draw, delta = self.plans, self.pushes - self._prev_pushes
        self.plans += 1
        usable = self._prev_usable and self._prev_x0 is not None and delta <= (self.pred_horizon - 1) * self.step_size
        warm = warm_start is not None and usable
        extra = {"candidates": K} if K > 1 else {}                             # 1: exactly the calls without the keyword
        guess, stride = None, 1
        if warm:
            i0 = N - int(warm_start)
            sa, sb = self._noise_level(i0)
            inp = self.model.prepare_inpaint_vectors(batch).contiguous() if self.inpaint_horizon > 0 else None
            if K > 1:                                                          # the previous plan K-fold: env_offset + row gives
                rep = lambda t: None if t is None else t.repeat_interleave(K, dim=0)  # noqa: E731  -- each candidate its noise
                x_start, guess, _ = self.warm_start(rep(self._prev_x0), rep(self._prev_translation), rep(batch["translation"]), rep(inp),
                                                    delta, sa, sb, seed, draw, return_parts=True)
                stride = K
            else:
                x_start = self.warm_start(self._prev_x0, self._prev_translation, batch["translation"], inp, delta, sa, sb, seed, draw)
            x_0 = self.model.sample(dict(batch), batched=True, sharded=False, seed=seed, x_T=x_start, start_step=i0, **extra)
        else:
            x_0 = self.model.sample(dict(batch), batched=True, sharded=False, seed=seed, x_T=x_T, **extra)
        x_0 = x_0.contiguous()
        picked = {}
        if K > 1:
            mode = "coherent" if usable and select != "medoid" else "medoid"
            rows = 0
            if mode == "coherent":
                rows = self.pred_horizon - delta // self.step_size - (1 if delta % self.step_size else 0)      # >= 1: `usable`
                if guess is None:                                              # the shifted previous plan alone: no noise enters it
                    inp = self.model.prepare_inpaint_vectors(batch).contiguous() if self.inpaint_horizon > 0 else None
                    guess = self.warm_start(self._prev_x0, self._prev_translation, batch["translation"], inp, delta, 1.0, 0.0, seed,
                                            draw, return_parts=True)[1]
            else:
                guess = None
            chosen, kept, scores, spread = self.select(x_0, K, mode, guess=guess, rows=rows, guess_row_stride=stride if guess is not None else 1,
                                                       cols=int(cols), translation=batch["translation"])
            if select == "first":
                chosen = torch.zeros_like(chosen)
                kept = x_0[0::K].contiguous()
            self.last_selection = {"scored_by": mode, "rows": rows, "cols": int(cols)}
            picked = dict(candidates=K, selected_by="first" if select == "first" else mode, chosen=chosen, scores=scores, spread=spread)
            x_0 = kept
        self._prev_x0, self._prev_translation = x_0, batch["translation"]
        self._prev_pushes, self._prev_usable = self.pushes, True
        out = self.unnormalize(x_0, batch["translation"])
        out.steps, out.warm = (int(warm_start) if warm else N), warm
        return out, picked


__all__ = ["CandidatePlan", "ClosedLoopPolicy", "Plan"]
