"""Host-side scheduler objects with the surface the reference's callers use on
diffusers' schedulers: construction kwargs (models/diffusion_ddpm.py:65-70,
generate.py:28-33), ``set_timesteps(n)``, ``.timesteps``,
``.config.num_train_timesteps`` and -- for callers that drive the loop themselves --
``step(eps, t, x).prev_sample`` / ``add_noise``.

They hold NO device code: they only produce the per-step coefficient table that
``spdm_set_schedule_tables`` (include/spdm.h) consumes, computed with torch fp32
scalars in the operation order of diffusers 0.17.1 so that the table is what the
reference's scheduler would use (the library can also build the table itself,
``spdm_set_schedule``; tests compare the two).

``DPMSolverMultistepScheduler`` is the exception to both: the reference never builds one, its table is computed in float64
numpy and rounded once, and the library has no built-in table for it.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from ._lib import SPDM_DDIM, SPDM_DDPM, SPDM_DPMPP_2M


class _LinearBetaScheduler:
    kind = -1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 1e-4, beta_end: float = 0.02,
                 beta_schedule: str = "linear", clip_sample: bool = False, prediction_type: str = "epsilon", **kw):
        if beta_schedule != "linear":
            raise NotImplementedError("the reference path only ever builds beta_schedule='linear' "
                                      "(models/diffusion_ddpm.py:67)")
        if clip_sample or prediction_type != "epsilon":
            raise NotImplementedError("reference path: clip_sample=False, prediction_type='epsilon'")
        self.config = SimpleNamespace(num_train_timesteps=int(num_train_timesteps), beta_start=beta_start,
                                      beta_end=beta_end, beta_schedule=beta_schedule, clip_sample=clip_sample,
                                      prediction_type=prediction_type, **kw)
        T = self.config.num_train_timesteps
        self.betas = torch.linspace(beta_start, beta_end, T, dtype=torch.float32)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.init_noise_sigma = 1.0
        self.num_inference_steps = T
        self.timesteps = torch.from_numpy(np.arange(0, T)[::-1].copy().astype(np.int64))
        self._device_tables = {}               # device_tables(): torch.device -> (sqrt(abar), sqrt(1 - abar))

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        if num_inference_steps > T:
            raise ValueError(f"num_inference_steps ({num_inference_steps}) > num_train_timesteps ({T})")
        self.num_inference_steps = int(num_inference_steps)
        ratio = T // self.num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts)

    def _prev(self, t: int) -> int:
        return t - self.config.num_train_timesteps // self.num_inference_steps

    def add_noise(self, original, noise, timesteps):
        acp = self.alphas_cumprod.to(original.device)
        sa = acp[timesteps] ** 0.5
        sb = (1 - acp[timesteps]) ** 0.5
        while sa.dim() < original.dim():
            sa, sb = sa.unsqueeze(-1), sb.unsqueeze(-1)
        return sa * original + sb * noise

    def device_tables(self, device):
        """``(sqrt(abar), sqrt(1 - abar))`` as (T,) fp32 tensors on ``device``, cached per device: ``add_noise``'s own
        expressions evaluated there over the whole table, so a gathered entry carries the bits ``add_noise`` computes."""
        device = torch.device(device)
        cache = self._device_tables
        if device not in cache:
            acp = self.alphas_cumprod.to(device)
            cache[device] = (acp ** 0.5, (1 - acp) ** 0.5)
        return cache[device]

    def coefficient_table(self) -> np.ndarray:
        """(n, 6) fp32: [sqrt(1-abar_t), sqrt(abar_t), k_x0, k_x, k_eps, k_noise] per loop iteration."""
        rows = [self._coef(int(t)) for t in self.timesteps.tolist()]
        return np.asarray(rows, dtype=np.float32)

    def step(self, model_output, timestep, sample, noise: Optional[torch.Tensor] = None, generator=None):
        c = [torch.tensor(v) for v in self._coef(int(timestep))]
        x0 = (sample - c[0] * model_output) / c[1]
        if self.kind == SPDM_DDPM:
            prev = c[2] * x0 + c[3] * sample
            if int(timestep) > 0:
                if noise is None:
                    noise = torch.randn(model_output.shape, generator=generator, dtype=model_output.dtype,
                                        device=model_output.device)
                prev = prev + c[5] * noise
        else:
            prev = c[2] * x0 + c[4] * model_output
        return SimpleNamespace(prev_sample=prev, pred_original_sample=x0)


class DDPMScheduler(_LinearBetaScheduler):
    """Stand-in for diffusers.schedulers.scheduling_ddpm.DDPMScheduler (0.17.1),
    epsilon prediction, fixed_small variance."""
    kind = SPDM_DDPM

    def _coef(self, t: int):
        prev_t = self._prev(t)
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        b_t = 1 - a_t
        b_prev = 1 - a_prev
        cur_a = a_t / a_prev
        cur_b = 1 - cur_a
        k_x0 = (a_prev ** 0.5 * cur_b) / b_t
        k_x = cur_a ** 0.5 * b_prev / b_t
        k_noise = torch.tensor(0.0)
        if t > 0:
            var = torch.clamp((1 - a_prev) / (1 - a_t) * cur_b, min=1e-20)
            k_noise = var ** 0.5
        return [float(b_t ** 0.5), float(a_t ** 0.5), float(k_x0), float(k_x), 0.0, float(k_noise)]


class DDIMScheduler(_LinearBetaScheduler):
    """Stand-in for diffusers.schedulers.scheduling_ddim.DDIMScheduler (0.17.1), eta = 0."""
    kind = SPDM_DDIM

    def _coef(self, t: int):
        prev_t = self._prev(t)
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t = 1 - a_t
        std = torch.tensor(0.0)
        k_eps = (1 - a_prev - std ** 2) ** 0.5
        return [float(b_t ** 0.5), float(a_t ** 0.5), float(a_prev ** 0.5), 0.0, float(k_eps), 0.0]


class DPMSolverMultistepScheduler(_LinearBetaScheduler):
    """DPM-Solver++ (2M): data prediction, multistep, midpoint (Lu et al. 2022, Algorithm 2), with the conventions of
    diffusers' ``DPMSolverMultistepScheduler`` RESTATED FROM MEMORY of release 0.17.1 -- diffusers is not a dependency and
    nothing here is pinned against it:

    * timesteps ``np.linspace(0, T - 1, n + 1).round()[::-1][:-1]``; the last step goes to timestep 0;
    * the first step of a loop is first order; with ``lower_order_final`` and n < 15 the last one is as well;
    * ``euler_at_final`` (a project extension under the name later diffusers releases use): the last step is first order
      for any n.

    With alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda_t = log alpha_t - log sigma_t, a step from timestep s
    to timestep t with h = lambda_t - lambda_s has ``k_x = sigma_t / sigma_s``, ``k0f = -alpha_t expm1(-h)`` and, after a
    step from s_prev, ``r = (lambda_s - lambda_s_prev) / h``, ``k0 = k0f (1 + 1 / (2 r))``, ``k1 = -k0f / (2 r)``:

        x0 = (x - sigma_s eps) / alpha_s
        first order :  x' = k_x x + k0f x0
        second order:  x' = k_x x + k0 x0 + k1 x0_prev

    ``coefficient_table()`` rows are ``{sigma_s, alpha_s, k_x, k0f, k0, k1}`` (a first-order row has k0 = k0f, k1 = 0),
    computed in float64 and rounded once to float32.  ``step`` is stateful: it keeps the previous call's x0 and runs first
    order whenever the previous call was not the loop iteration just before (``set_timesteps`` forgets it)."""
    kind = SPDM_DPMPP_2M

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 1e-4, beta_end: float = 0.02,
                 beta_schedule: str = "linear", solver_order: int = 2, algorithm_type: str = "dpmsolver++",
                 solver_type: str = "midpoint", lower_order_final: bool = True, euler_at_final: bool = False,
                 prediction_type: str = "epsilon", thresholding: bool = False):
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order = {solver_order!r}: orders 1 and 2 only")
        if algorithm_type != "dpmsolver++" or solver_type != "midpoint":
            raise NotImplementedError("algorithm_type='dpmsolver++' with solver_type='midpoint' only")
        if thresholding:
            raise NotImplementedError("thresholding=False only")
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                         beta_schedule=beta_schedule, prediction_type=prediction_type, solver_order=int(solver_order),
                         algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=bool(lower_order_final),
                         euler_at_final=bool(euler_at_final), thresholding=False)
        T = self.config.num_train_timesteps
        abar = np.cumprod(1.0 - np.linspace(float(beta_start), float(beta_end), T, dtype=np.float64))
        self._alpha, self._sigma = np.sqrt(abar), np.sqrt(1.0 - abar)
        self._lambda = np.log(self._alpha) - np.log(self._sigma)
        self._table = None
        self._last = (None, None)              # step(): (loop iteration, x0) of the previous call
        self.set_timesteps(max(T - 1, 1))

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, n = self.config.num_train_timesteps, int(num_inference_steps)
        if n < 1:
            raise ValueError(f"num_inference_steps ({n}) must be >= 1")
        ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        if np.unique(ts).size != n:
            raise ValueError(f"num_inference_steps = {n} repeats a timestep on a grid of {T}")
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(ts)
        self._table, self._last = None, (None, None)

    def _rows(self) -> np.ndarray:
        """(n, 6) float64: {sigma_s, alpha_s, k_x, k0f, k0, k1} per loop iteration."""
        cfg, ts = self.config, self.timesteps.tolist()
        n = len(ts)
        al, sg, lam = self._alpha, self._sigma, self._lambda
        rows = np.zeros((n, 6), dtype=np.float64)
        for i, s in enumerate(ts):
            t = ts[i + 1] if i + 1 < n else 0
            h = lam[t] - lam[s]
            k0f = -al[t] * np.expm1(-h)
            final_first = i == n - 1 and (cfg.euler_at_final or (cfg.lower_order_final and n < 15))
            if i == 0 or cfg.solver_order == 1 or final_first:
                k0, k1 = k0f, 0.0
            else:
                r = (lam[s] - lam[ts[i - 1]]) / h
                k0, k1 = k0f * (1.0 + 1.0 / (2.0 * r)), -k0f / (2.0 * r)
            rows[i] = (sg[s], al[s], sg[t] / sg[s], k0f, k0, k1)
        return rows

    def coefficient_table(self) -> np.ndarray:
        """(n, 6) fp32: [sigma_s, alpha_s, k_x, k0f, k0, k1] per loop iteration."""
        if self._table is None:
            self._table = self._rows().astype(np.float32)
        return self._table

    def step(self, model_output, timestep, sample, **kw):
        ts = self.timesteps.tolist()
        i = ts.index(int(timestep))
        c = [torch.tensor(v) for v in self.coefficient_table()[i]]
        x0 = (sample - c[0] * model_output) / c[1]
        prev = c[2] * sample
        if self._last[0] != i - 1 or i == 0 or float(c[5]) == 0.0:
            prev = prev + c[3] * x0
        else:
            prev = prev + c[4] * x0
            prev = prev + c[5] * self._last[1]
        self._last = (i, x0)
        return SimpleNamespace(prev_sample=prev, pred_original_sample=x0)
