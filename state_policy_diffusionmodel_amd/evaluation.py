"""Position and action error of a trained model over a dataset, measured on the device.

Replaces the reference's evaluation/eval_acurracy_diffusion_positions.py (every window of a dataset) and
evaluation/eval_consistency_diffusion_positions.py (repeated runs of one window): there each trajectory is a B = 1
``model.sample``, a ``.cpu()``, and numpy's ``unnormalize_position`` / ``np.linalg.norm``.  Here the trajectories of all windows
and runs are sampled in chunks of ``batch_size``, ``spdm_eval_errors`` (csrc/evaluation.hip) turns each chunk's x_0 into errors
in one launch, and ``spdm_eval_reduce`` forms the statistics; only the errors and their statistics travel to the host, once.

There is no CPU fallback: ``evaluate`` needs the GPU."""
from __future__ import annotations

import ctypes
import json
import math
from dataclasses import dataclass
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .dataset import DeviceDataset


@dataclass
class EvalReport:
    """numpy float64 arrays; K windows, ``runs`` trajectories each, P = pred_horizon.  ``mean_error`` / ``std_error`` are the
    curves the reference's two scripts plot (over all K * runs rows), ``window_mean`` / ``window_std`` the same over the runs
    of each window.  The ``action_*`` fields (a trailing axis of 3 channels) are None when actions were not evaluated."""
    window_ids: np.ndarray                     # (K,) int64
    runs: int
    seed: int
    position_error: np.ndarray                 # (K, runs, P)
    mean_error: np.ndarray                     # (P,)
    std_error: np.ndarray                      # (P,)
    window_mean: np.ndarray                    # (K, P)
    window_std: np.ndarray                     # (K, P)
    action_error: Optional[np.ndarray] = None          # (K, runs, P, 3)
    action_mean_error: Optional[np.ndarray] = None     # (P, 3)
    action_std_error: Optional[np.ndarray] = None      # (P, 3)
    action_window_mean: Optional[np.ndarray] = None    # (K, P, 3)
    action_window_std: Optional[np.ndarray] = None     # (K, P, 3)

    ARRAYS = ("position_error", "mean_error", "std_error", "window_mean", "window_std", "action_error", "action_mean_error",
              "action_std_error", "action_window_mean", "action_window_std")

    def to_dict(self) -> dict:
        d = {"window_ids": self.window_ids.tolist(), "runs": self.runs, "seed": self.seed}
        for k in self.ARRAYS:
            v = getattr(self, k)
            d[k] = None if v is None else v.tolist()
        return d

    def to_json(self, **kw) -> str:
        return json.dumps(self.to_dict(), **kw)


def initial_noise(model, n: int, seed: int) -> torch.Tensor:
    """x_T of all ``n`` trajectories, (n, 1, H, D) uniform like the reference's (models/diffusion_ddpm.py:252), drawn ONCE
    from a device generator seeded by ``seed``: a chunk takes its slice, so x_T does not depend on ``batch_size``."""
    gen = torch.Generator(device=model.device).manual_seed(int(seed))
    H = model.pred_horizon + model.inpaint_horizon
    return torch.rand(n, 1, H, model.prediction_dim, device=model.device, generator=gen)


def chunks(n_windows: int, runs: int, batch_size: int) -> Iterator[Tuple[int, int, int, int]]:
    """``(g0, g1, k0, k1)``: trajectories [g0, g1) (trajectory g is run g % runs of window g // runs) and the windows
    [k0, k1) they touch; a boundary may fall inside a window's runs."""
    N = n_windows * runs
    for g0 in range(0, N, batch_size):
        g1 = min(N, g0 + batch_size)
        yield g0, g1, g0 // runs, (g1 - 1) // runs + 1


def _position_stats(stats) -> Tuple[float, float]:
    return float(stats["position"]["min"]), float(stats["position"]["max"])


def _action_stats(stats):
    lo, hi = (np.asarray(stats["action"][k], dtype=np.float64).reshape(-1) for k in ("min", "max"))
    if lo.shape != (3,) or hi.shape != (3,):
        raise ValueError(f"action statistics must have 3 channels, got {lo.shape} and {hi.shape}")
    return lo, hi


def errors_into(pred: torch.Tensor, batch: dict, stats: dict, *, obs_h: int, inp_h: int, runs: int, first_traj: int,
                window_base: int, pos_err: torch.Tensor, act_err: Optional[torch.Tensor] = None) -> None:
    """One ``spdm_eval_errors`` launch on torch's current stream: ``pred`` (B, 1, H, D) or (B, H, D), the sampler's x_0 of
    trajectories ``first_traj ..``, against ``batch`` (a ``DeviceDataset.batch(..., with_translation=True)`` of windows
    ``window_base ..``) into ``pos_err`` (B, P) and, if given, ``act_err`` (B, P, 3), float64 device tensors."""
    if pred.dim() == 4:
        pred = pred[:, 0]
    B, H, D = pred.shape
    P = pos_err.shape[1]
    tp, tr, ta = batch["position"], batch["translation"], batch["action"] if act_err is not None else None
    for name, t, dt in (("pred", pred, torch.float32), ("position", tp, torch.float32), ("translation", tr, torch.float64),
                        ("action", ta, torch.float32), ("pos_err", pos_err, torch.float64), ("act_err", act_err, torch.float64)):
        if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dt} device tensor")
    if pos_err.shape != (B, P) or (act_err is not None and act_err.shape != (B, P, 3)):
        raise ValueError(f"pos_err must be (B, P) = ({B}, {P}) and act_err (B, P, 3)")
    n_slots, seq = tp.shape[0], tp.shape[1]
    if tp.shape != (n_slots, seq, 2) or tr.shape != (n_slots, 2) or (ta is not None and ta.shape != (n_slots, seq, 3)):
        raise ValueError("batch must hold position (n, seq, 2), translation (n, 2) and action (n, seq, 3)")
    pos_min, pos_max = _position_stats(stats)
    a = _lib.SpdmEvalErrorsArgs(B=B, H=H, D=D, n_slots=n_slots, seq=seq, obs_h=obs_h, inp_h=inp_h, P=P, runs=runs,
                                window_base=window_base, first_traj=first_traj, d_pred=pred.data_ptr(), d_truth_pos=tp.data_ptr(),
                                d_truth_act=ta.data_ptr() if ta is not None else None, d_translation=tr.data_ptr(),
                                pos_min=pos_min, pos_max=pos_max, d_pos_err=pos_err.data_ptr(),
                                d_act_err=act_err.data_ptr() if act_err is not None else None)
    if act_err is not None:
        lo, hi = _action_stats(stats)
        a.act_min[:], a.act_max[:] = lo.tolist(), hi.tolist()
    stream = ctypes.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
    _lib.check(_lib.load().spdm_eval_errors(pred.device.index, ctypes.byref(a), stream), "spdm_eval_errors")


def reduce_errors(err: torch.Tensor, runs: int):
    """``spdm_eval_reduce`` over ``err`` (N, C) float64 on the device, N = windows * runs: device tensors ``(window_mean
    (N / runs, C), window_std, mean (C), std)``, enqueued on torch's current stream."""
    if not err.is_cuda or err.dtype != torch.float64 or err.dim() != 2 or not err.is_contiguous():
        raise ValueError("err must be a contiguous (N, C) float64 device tensor")
    N, C = err.shape
    if runs < 1 or N < 1 or N % runs:
        raise ValueError(f"N = {N} rows are not windows x runs = {runs}")
    lib = _lib.load()
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=err.device)  # noqa: E731
    wmean, wstd, mean, std = f64(N // runs, C), f64(N // runs, C), f64(C), f64(C)
    n_ws = int(lib.spdm_eval_reduce_workspace_doubles(N, C))
    ws = f64(max(n_ws, 1))
    a = _lib.SpdmEvalReduceArgs(N=N, C=C, runs=runs, d_err=err.data_ptr(), d_window_mean=wmean.data_ptr(), d_window_std=wstd.data_ptr(),
                                d_mean=mean.data_ptr(), d_std=std.data_ptr(), d_workspace=ws.data_ptr(), workspace_doubles=n_ws)
    stream = ctypes.c_void_p(torch.cuda.current_stream(err.device).cuda_stream)
    _lib.check(lib.spdm_eval_reduce(err.device.index, ctypes.byref(a), stream), "spdm_eval_reduce")
    return wmean, wstd, mean, std


def _check(model, dataset: DeviceDataset, window_ids, runs: int, batch_size: int, actions: bool) -> np.ndarray:
    """The argument checks ``evaluate`` and ``robustness`` share; the window ids as an int64 array."""
    if runs < 1 or batch_size < 1:
        raise ValueError(f"runs = {runs} and batch_size = {batch_size} must be >= 1")
    obs_h, P, inp_h, D = model.obs_horizon, model.pred_horizon, model.inpaint_horizon, model.prediction_dim
    if (dataset.obs_horizon, dataset.pred_horizon) != (obs_h, P):
        raise ValueError(f"the dataset's windows are obs {dataset.obs_horizon} + pred {dataset.pred_horizon}, the model's "
                         f"obs {obs_h} + pred {P}")
    if inp_h > obs_h:
        raise ValueError(f"inpaint_horizon = {inp_h} exceeds obs_horizon = {obs_h}")
    if D < (5 if actions else 2):
        raise ValueError(f"prediction_dim = {D} holds no {'action (pass actions=False)' if D >= 2 else 'position'}")
    if dataset.device != model.device:
        raise ValueError(f"dataset on {dataset.device}, model on {model.device}")
    ids = np.arange(len(dataset), dtype=np.int64) if window_ids is None else np.asarray(window_ids).reshape(-1)
    if ids.size == 0 or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError("window_ids must be a non-empty list of integers")
    ids = ids.astype(np.int64)
    if ids.min() < 0 or ids.max() >= len(dataset):
        raise IndexError(f"window id {int(ids[(ids < 0) | (ids >= len(dataset))][0])} outside [0, {len(dataset)})")
    return ids


def _sample_chunk(model, observed: dict, x_T: torch.Tensor, runs: int, seed: int, g0: int, g1: int, k0: int) -> torch.Tensor:
    """x_0 of trajectories [g0, g1), conditioned on ``observed``: the batch dict of the windows ``k0 ..`` they belong to."""
    observation = model.prepare_observation_batch(observed)
    obs_cond = model.prepare_obs_cond_vectors(observation)                         # once per window ...
    inpaint = model.prepare_inpaint_vectors(observation)
    slot = torch.div(torch.arange(g0, g1, device=model.device), runs, rounding_mode="floor") - k0
    x_0 = model.sample({"obs_cond": obs_cond.index_select(0, slot), "inpaint": inpaint.index_select(0, slot)},       # ... per run
                       batched=True, sharded=False, x_T=x_T[g0:g1], seed=seed, sample_offset=g0)
    return x_0.contiguous()


def _statistics(pos_err: torch.Tensor, act_err: Optional[torch.Tensor], K: int, runs: int, P: int) -> dict:
    """``EvalReport``'s arrays as device tensors, from the error buffers of K * runs trajectories."""
    N, rep = K * runs, {}
    for prefix, err, tail in (("", pos_err, ()),) + ((("action_", act_err, (3,)),) if act_err is not None else ()):
        wmean, wstd, mean, std = reduce_errors(err.view(N, -1), runs)
        rep[prefix + "window_mean"], rep[prefix + "window_std"] = wmean.view((K, P) + tail), wstd.view((K, P) + tail)
        rep[prefix + "mean_error"], rep[prefix + "std_error"] = mean.view((P,) + tail), std.view((P,) + tail)
        rep["action_error" if prefix else "position_error"] = err.view((K, runs, P) + tail)
    return rep


def _read_back(rep: dict) -> dict:
    """Every device tensor of ``rep`` as a numpy array, through ONE copy to the host."""
    host = torch.cat([v.reshape(-1) for v in rep.values()]).cpu().numpy()
    out, at = {}, 0
    for k, v in rep.items():
        out[k] = host[at:at + v.numel()].reshape(tuple(v.shape)).copy()
        at += v.numel()
    return out


def evaluate(model, dataset: DeviceDataset, window_ids=None, runs: int = 10, batch_size: int = 4096, seed: int = 0,
             actions: bool = True) -> EvalReport:
    """Sample ``runs`` trajectories for each window of ``window_ids`` (default: every window of ``dataset``) with ``model`` (a
    ``Diffusion_DDPM`` / ``Diffusion_DDIM``) and measure, per predicted step, the distance between the predicted and the true
    position in the dataset's units, and with ``actions=True`` the absolute error of each action channel.

    Trajectory ``g = k * runs + r`` is run ``r`` of ``window_ids[k]``; its x_T is row ``g`` of ``initial_noise(model, K * runs,
    seed)`` and its step noise is keyed by ``(seed, g)``, so the report is a function of (weights, data, ids, runs, seed) and not
    of ``batch_size`` -- up to fp32 rounding, because the sampler selects its kernels by batch size."""
    if not isinstance(dataset, DeviceDataset):
        raise TypeError("dataset must be a DeviceDataset")
    runs, batch_size, seed = int(runs), int(batch_size), int(seed)
    ids = _check(model, dataset, window_ids, runs, batch_size, actions)
    obs_h, P, inp_h = model.obs_horizon, model.pred_horizon, model.inpaint_horizon
    K = len(ids)
    N = K * runs
    dev = model.device
    d_ids = torch.from_numpy(ids.astype(np.int32)).to(dev)
    x_T = initial_noise(model, N, seed)
    pos_err = torch.empty((N, P), dtype=torch.float64, device=dev)
    act_err = torch.empty((N, P, 3), dtype=torch.float64, device=dev) if actions else None
    for g0, g1, k0, k1 in chunks(K, runs, batch_size):
        batch = dataset.batch(d_ids[k0:k1], frames="obs", with_translation=True)
        x_0 = _sample_chunk(model, batch, x_T, runs, seed, g0, g1, k0)
        errors_into(x_0, batch, dataset.stats, obs_h=obs_h, inp_h=inp_h, runs=runs, first_traj=g0, window_base=k0,
                    pos_err=pos_err[g0:g1], act_err=act_err[g0:g1] if actions else None)
    return EvalReport(window_ids=ids, runs=runs, seed=seed, **_read_back(_statistics(pos_err, act_err, K, runs, P)))   # one read-back


@dataclass
class RobustnessReport:
    """``EvalReport``'s arrays with a leading axis of L noise levels, and the two curves the reference's
    evaluation/eval_robustness.py:313-318 computes: ``mse_position[lev]`` is the mean over windows, runs, steps and both
    coordinates of the squared position error (dataset units squared), ``mse_action[lev]`` the mean over windows, runs, steps and
    the three channels of the squared action error."""
    levels: np.ndarray                         # (L,) float64: alpha of each level (the kernel takes it rounded to float32)
    draws: np.ndarray                          # (L,) int64: the Philox draw word of each level
    window_ids: np.ndarray                     # (K,) int64
    runs: int
    seed: int
    mse_position: np.ndarray                   # (L,)
    mse_action: np.ndarray                     # (L,)
    position_error: np.ndarray                 # (L, K, runs, P)
    mean_error: np.ndarray                     # (L, P)
    std_error: np.ndarray                      # (L, P)
    window_mean: np.ndarray                    # (L, K, P)
    window_std: np.ndarray                     # (L, K, P)
    action_error: np.ndarray                   # (L, K, runs, P, 3)
    action_mean_error: np.ndarray              # (L, P, 3)
    action_std_error: np.ndarray               # (L, P, 3)
    action_window_mean: np.ndarray             # (L, K, P, 3)
    action_window_std: np.ndarray              # (L, K, P, 3)

    ARRAYS = EvalReport.ARRAYS

    def level(self, lev: int) -> EvalReport:
        """Level ``lev`` as the ``EvalReport`` that ``evaluate`` would return for observations perturbed that much."""
        return EvalReport(window_ids=self.window_ids, runs=self.runs, seed=self.seed, **{k: getattr(self, k)[lev] for k in self.ARRAYS})

    def to_dict(self) -> dict:
        d = {"levels": self.levels.tolist(), "draws": self.draws.tolist(), "window_ids": self.window_ids.tolist(), "runs": self.runs,
             "seed": self.seed, "mse_position": self.mse_position.tolist(), "mse_action": self.mse_action.tolist()}
        d.update({k: getattr(self, k).tolist() for k in self.ARRAYS})
        return d

    def to_json(self, **kw) -> str:
        return json.dumps(self.to_dict(), **kw)


DEFAULT_LEVELS = tuple(round(0.01 * k, 2) for k in range(10))     # eval_robustness.py:166-175: run * 0.01, ten runs


def mean_square(column_means, divisor: int = 1) -> float:
    """The mean of a squared-error buffer from its column means (``reduce_errors`` over the squares; every column has the same
    number of rows), combined exactly with ``math.fsum``.  ``divisor = 2`` for the position: the squared distance is the sum of
    two squared coordinates, and the reference's ``np.mean(np.square(pred - truth))`` averages over both."""
    m = np.asarray(column_means, dtype=np.float64).reshape(-1)
    return math.fsum(m.tolist()) / (m.size * divisor)


def robustness(model, dataset: DeviceDataset, window_ids=None, levels=DEFAULT_LEVELS, draws=None, runs: int = 1,
               batch_size: int = 4096, seed: int = 0) -> RobustnessReport:
    """``evaluate`` under observation noise: for each ``levels[lev]`` the frames, positions, velocities and actions a window's
    prediction is conditioned on (and its in-painted rows are taken from) get ``levels[lev] * U[0, 1)`` added
    (``noising.perturb_observations``), and the errors against the CLEAN truth are measured as ``evaluate`` does.

    Every level perturbs the clean observations: nothing accumulates from level to level (the reference's loop adds each run's
    noise onto the last one's batch).  Level ``lev`` of window ``window_ids[k]`` draws Philox stream
    ``(seed, draws[lev], k)``, ``draws`` defaulting to ``0 .. L - 1``; the runs of a window share the perturbation and differ by
    the sampler's noise.  x_T and the sampler's noise are those of ``evaluate(..., seed=seed)`` at every level, so levels differ
    by the observation noise alone, and a level of 0 launches nothing and is ``evaluate`` bit for bit."""
    from .noising import perturb_observations
    if not isinstance(dataset, DeviceDataset):
        raise TypeError("dataset must be a DeviceDataset")
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    dr = np.arange(lv.size, dtype=np.int64) if draws is None else np.asarray(draws).reshape(-1)
    if lv.size == 0 or dr.size != lv.size:
        raise ValueError(f"{lv.size} levels and {dr.size} draws: one draw per level, at least one level")
    if not np.isfinite(lv).all() or lv.min() < 0:
        raise ValueError(f"levels must be finite and >= 0, got {lv.tolist()}")
    if not np.issubdtype(dr.dtype, np.integer) or dr.min() < 0 or dr.max() > 0xFFFFFFFF:
        raise ValueError("draws must be integers in [0, 2^32)")
    dr = dr.astype(np.int64)
    runs, batch_size, seed = int(runs), int(batch_size), int(seed)
    ids = _check(model, dataset, window_ids, runs, batch_size, True)
    obs_h, P, inp_h = model.obs_horizon, model.pred_horizon, model.inpaint_horizon
    K, L = len(ids), lv.size
    N = K * runs
    dev = model.device
    d_ids = torch.from_numpy(ids.astype(np.int32)).to(dev)
    x_T = initial_noise(model, N, seed)
    pos_err = torch.empty((L, N, P), dtype=torch.float64, device=dev)
    act_err = torch.empty((L, N, P, 3), dtype=torch.float64, device=dev)
    for g0, g1, k0, k1 in chunks(K, runs, batch_size):
        batch = dataset.batch(d_ids[k0:k1], frames="obs", with_translation=True)     # gathered once for all levels
        for lev in range(L):
            observed = batch if lv[lev] == 0 else perturb_observations(batch, float(lv[lev]), obs_horizon=obs_h, seed=seed, draw=int(dr[lev]),
                                                                     row_offset=k0)
            x_0 = _sample_chunk(model, observed, x_T, runs, seed, g0, g1, k0)
            errors_into(x_0, batch, dataset.stats, obs_h=obs_h, inp_h=inp_h, runs=runs, first_traj=g0, window_base=k0,
                        pos_err=pos_err[lev, g0:g1], act_err=act_err[lev, g0:g1])
    per_level = [_statistics(pos_err[lev], act_err[lev], K, runs, P) for lev in range(L)]
    rep = {k: torch.stack([r[k] for r in per_level]) for k in per_level[0]}
    rep["pos_sq"] = torch.stack([reduce_errors((pos_err[lev] * pos_err[lev]).view(N, -1), runs)[2] for lev in range(L)])       # (L, P)
    rep["act_sq"] = torch.stack([reduce_errors((act_err[lev] * act_err[lev]).view(N, -1), runs)[2] for lev in range(L)])       # (L, 3 P)
    out = _read_back(rep)                                                              # the one read-back
    pos_sq, act_sq = out.pop("pos_sq"), out.pop("act_sq")
    return RobustnessReport(levels=lv, draws=dr, window_ids=ids, runs=runs, seed=seed,
                            mse_position=np.array([mean_square(pos_sq[lev], 2) for lev in range(L)]),
                            mse_action=np.array([mean_square(act_sq[lev]) for lev in range(L)]), **out)


__all__ = ["EvalReport", "RobustnessReport", "evaluate", "robustness", "mean_square", "initial_noise", "chunks", "errors_into",
           "reduce_errors", "DEFAULT_LEVELS"]
