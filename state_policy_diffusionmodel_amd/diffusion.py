"""Host-side mirror of the reference's sampler objects for the hot path:
``Diffusion_DDPM`` (``/root/reference/models/diffusion_ddpm.py:22-88, 216-277, 283-348``) and
``Diffusion_DDIM`` (``models/diffusion_ddim.py:19-74``).

Same constructor keywords, same attributes a caller touches (``noise_scheduler``,
``noise_steps``, ``noise_estimator``, ``obs_horizon``, ``pred_horizon``, ``inpaint_horizon``,
``prediction_dim``, ``vision_encoder``), same ``sample(batch, option)`` signature and return
types -- so ``generate.py``'s idiom

    model.noise_scheduler = DDIMScheduler(num_train_timesteps=100, ...)   # generate.py:28-34
    model.noise_steps = 100                                               # generate.py:35
    history = model.sample(batch=obs, option='sample_history')            # generate.py:73-76

works unchanged.  What runs underneath is libspdm_hip.so (no torch compute in the loop).
Validation plots and the Lightning plumbing are out of scope.

All three noise predictors of ``__init__`` (models/diffusion_ddpm.py:53-62) run on that path: ``model='UNet_Film'``,
``'UNet_FilmnoAttention'``, and every other value -- the constructor's own default ``'UNet'`` -- for
models/simple_Unet.py's concat-conditioned ``UNet``.  Evaluation always has eval semantics: that network's
positional-encoding dropout is off, as in the reference's ``validation_step`` and ``sample()`` after ``model.eval()``;
the reference's ``training_step`` runs it with dropout p = 0.1, which ``training_step(..., backward=True,
time_scale=mask)`` reproduces when the caller draws the mask (otherwise its forward half is the eval-mode network).
``training_step(..., backward=True)`` also computes the gradients, for ``'UNet_FilmnoAttention'``
(``spdm_train_loss_grad``), for simple_Unet.py's ``'UNet'`` and -- constructed with
``train_attention=True`` -- ``'UNet_Film'``; the optimiser is torch's, or -- ``configure_optimizers(device_optimizer=True)`` --
``optim.DeviceAdam`` in HIP.  ``train_vision_encoder=True`` is the reference's
joint training of the frame encoder (``Adam(self.parameters())``, :115-116): the step then also
backpropagates into ``vision_encoder`` and the optimiser steps both.

Explicit, non-breaking extensions: ``sample(..., x_T=, noise=, batched=, seed=)`` for
fixed-noise parity runs and for B > 1 independent trajectories (the reference hard-wires
B = 1 by taking ``obs_cond[0]``, ``models/diffusion_ddpm.py:246``).
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, List, Optional

import numpy as np

import torch

from .engine import SpdmEngine
from .schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, _LinearBetaScheduler
from .weights import is_simple_model, pack_state_dict, random_state_dict, state_dict_to_numpy


def _as_spec(sched) -> _LinearBetaScheduler:
    """Accept our own scheduler objects, or a diffusers-like one (duck-typed on class name and
    ``config``), as ``generate.py`` may assign either."""
    if isinstance(sched, _LinearBetaScheduler):
        return sched
    name = type(sched).__name__
    cfg = getattr(sched, "config", None)
    T = getattr(cfg, "num_train_timesteps", None) if cfg is not None else None
    if T is None:
        raise TypeError(f"cannot interpret noise_scheduler of type {name}")
    kw = dict(num_train_timesteps=int(T), beta_start=float(getattr(cfg, "beta_start", 1e-4)),
              beta_end=float(getattr(cfg, "beta_end", 0.02)),
              beta_schedule=getattr(cfg, "beta_schedule", "linear"),
              clip_sample=bool(getattr(cfg, "clip_sample", False)),
              prediction_type=getattr(cfg, "prediction_type", "epsilon"))
    if "DPMSolverMultistep" in name:
        if getattr(cfg, "use_karras_sigmas", False) or getattr(cfg, "trained_betas", None) is not None:
            raise NotImplementedError("DPMSolverMultistepScheduler: use_karras_sigmas and trained_betas are not supported")
        del kw["clip_sample"]
        opts = {k: getattr(cfg, k) for k in ("solver_order", "algorithm_type", "solver_type", "lower_order_final", "euler_at_final",
                                             "thresholding") if hasattr(cfg, k)}
        return DPMSolverMultistepScheduler(**kw, **opts)
    if "DDIM" in name:
        return DDIMScheduler(**kw)
    if "DDPM" in name:
        return DDPMScheduler(**kw)
    raise TypeError(f"unsupported scheduler class {name} (DDPM / DDIM / DPMSolverMultistep only)")


def _index_of(idx):
    """The layout of a packed state_dict (weights.pack_state_dict): [(name, offset, shape)]."""
    return [(e.name.decode(), int(e.offset), tuple(e.shape[d] for d in range(e.ndim))) for e in idx]


class NoiseEstimator:
    """``self.noise_estimator`` of the reference (``UNet_Film(...)`` built at
    models/diffusion_ddpm.py:76-82): holds the weights; calling it evaluates the HIP U-Net."""

    def __init__(self, owner: "Diffusion_DDPM", state_dict):
        self._owner = owner
        self._host_sd = state_dict_to_numpy(state_dict)
        self._flat: Optional[torch.nn.Parameter] = None     # flat_parameter(): the packed state_dict on the device
        self._flat_index = None                             # ... its layout [(name, offset, shape)]
        self._flat_version = 0                              # ... its torch version when _host_sd last matched it

        self._grads: Optional[Dict[str, torch.Tensor]] = None
        self.grad_cond: Optional[torch.Tensor] = None

    @property
    def _sd(self) -> Dict[str, np.ndarray]:
        """The host copy of the weights, brought up to date from ``flat_parameter()`` when an optimiser changed it."""
        if self._flat is not None and self._flat._version != self._flat_version:
            self._host_sd = self._unpack(self._flat)
            self._flat_version = self._flat._version
        return self._host_sd

    def _unpack(self, flat: torch.Tensor) -> Dict[str, np.ndarray]:
        """A device tensor in ``flat_parameter()``'s layout as name -> host array (copies)."""
        host = flat.detach().cpu().numpy()
        sd = {}
        for name, off, shape in self._flat_index:
            n = int(np.prod(shape)) if shape else 1
            sd[name] = host[off:off + n].reshape(shape).copy()
        return sd

    def state_dict(self):
        return {k: torch.from_numpy(v) for k, v in self._sd.items()}

    def mark_moved(self) -> None:
        """``flat_parameter()`` was written behind torch's back (``DeviceAdam`` steps it through its pointer, which does not
        advance the tensor's version): the host copy is fetched again on its next use."""
        self._flat_version = None

    def _engines(self):
        return [e for e in (self._owner._engine, self._owner._train_engine) if e is not None]

    def load_state_dict(self, state_dict) -> None:
        """Replace the weights (e.g. after an optimiser step) and push them into every engine the owner has cached: packed
        and uploaded once, then put into each engine in place (SpdmEngine.update_weights); an engine whose packed layout
        differs is rebuilt (SpdmEngine.refresh_weights).  ``flat_parameter()``, if created, takes the new values."""
        self._host_sd = state_dict_to_numpy(state_dict)
        blob, idx = pack_state_dict(self._host_sd)
        index = _index_of(idx)
        dev = None
        for eng in self._engines():
            if eng._index == index:
                if dev is None:
                    dev = torch.from_numpy(blob).to(eng.device)
                eng.update_weights(dev)
            else:
                eng.refresh_weights(self._host_sd)
        if self._flat is not None:
            if index == self._flat_index:
                with torch.no_grad():
                    self._flat.copy_(torch.from_numpy(blob).to(self._flat.device))
                self._flat_version = self._flat._version
            else:
                self._flat = None

    def flat_parameter(self) -> torch.nn.Parameter:
        """The weights as ONE device parameter in the packed state_dict layout (``SpdmEngine.pack_weights``), created on
        first use; the optimiser of ``Diffusion_DDPM.configure_optimizers`` steps it.  After
        ``training_step(backward=True)`` its ``.grad`` is the flat gradient, and ``grads()`` are views of that storage."""
        if self._flat is None:
            blob, idx = pack_state_dict(self._host_sd)
            self._flat = torch.nn.Parameter(torch.from_numpy(blob).to(self._owner.device))
            self._flat_index = _index_of(idx)
            self._flat_version = self._flat._version
        return self._flat

    def _push(self, other: Optional[torch.Tensor] = None, engines=None) -> None:
        """Put ``flat_parameter()``'s values into every cached engine (in place where the layout matches).  ``other``: a device
        tensor in the flat parameter's layout whose values go in instead (the EMA shadow, ``Diffusion_DDPM.ema_weights``);
        the flat parameter and the host copy stay as they are.  ``engines``: these engines only."""
        flat = self._flat.detach() if other is None else other.detach()
        for eng in (self._engines() if engines is None else engines):
            if eng._index == self._flat_index:
                eng.update_weights(flat)
            else:
                eng.refresh_weights(self._sd if other is None else self._unpack(flat))

    def grads(self) -> Dict[str, torch.Tensor]:
        """Gradients of the loss of the last ``training_step(..., backward=True)``: state_dict name -> tensor (torch layout,
        on the device), as ``{n: p.grad for n, p in noise_estimator.named_parameters()}`` after ``loss.backward()``.
        ``grad_cond`` holds d loss / d obs_cond of that step (None without conditioning)."""
        if self._grads is None:
            raise RuntimeError("no gradients: call training_step(..., backward=True) first")
        return self._grads

    def __call__(self, x: torch.Tensor, t: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
        eng = self._owner._engine_for(x.shape[0], x.shape[-2], x.shape[-1])
        return eng.unet_forward(x, t, y)


class Diffusion_DDPM:
    def __init__(self, noise_steps: int = 1000, obs_horizon: int = 10, pred_horizon: int = 10,
                 observation_dim: int = 2, prediction_dim: int = 2, learning_rate: float = 1e-4,
                 model: str = "UNet", vision_encoder: Optional[Callable] = None,
                 noise_scheduler_type: str = "linear", inpaint_horizon: int = 10, step_size: int = 1,
                 *, state_dict=None, weight_seed: int = 0, device: int = 0, max_batch: int = 1,
                 vision_encoder_state_dict=None, train_attention: bool = False, train_vision_encoder: bool = False):
        # --- Diffusion params (models/diffusion_ddpm.py:42-48)
        self.noise_steps = noise_steps
        self.obs_horizon = obs_horizon
        self.pred_horizon = pred_horizon
        self.observation_dim = observation_dim
        self.prediction_dim = prediction_dim
        self.inpaint_horizon = inpaint_horizon
        self.lr = learning_rate
        self.noise_scheduler_type = noise_scheduler_type   # (kept for hparams.yaml only: the reference ignores it, :65-70)
        self.step_size = step_size
        # --- architecture switch (:54-62): every name but the two FiLM ones builds simple_Unet.UNet
        self.model_name = model
        self.simple = is_simple_model(model)
        self.attention = model == "UNet_Film"
        self.train_attention = bool(train_attention)      # training_step(backward=True) for UNet_Film (SPDM_FLAG_TRAIN_ATTENTION)
        self._noise_step = 0                               # training_step(device_noise=True, noise_step=None): its own step counter
        self._fp_spec = (None, None)                       # forward_process: (noise_scheduler object, its _LinearBetaScheduler)
        # --- scheduler (:65-70); beta schedule is hard-coded 'linear' there, noise_scheduler_type unused
        self.noise_scheduler = DDPMScheduler(num_train_timesteps=self.noise_steps, beta_schedule="linear",
                                             clip_sample=False, prediction_type="epsilon")
        self.cond_dim = observation_dim * obs_horizon
        if state_dict is None:   # random-init, like constructing the reference module without a checkpoint
            state_dict = random_state_dict(self.cond_dim, seed=weight_seed, attention=self.attention,
                                           model=model, noise_steps=self.noise_steps)
        self.noise_estimator = NoiseEstimator(self, state_dict)
        # the reference loads a private autoencoder checkpoint here (:84-88).  Given that encoder's tensors
        # (vision_encoder_state_dict: keys 0.weight .. 7.bias, as in the diffusion checkpoint's 'vision_encoder.*'), the
        # front end runs in libspdm_hip.so (vision.VisionEncoder, built on first use); any other callable
        # (N,3,96,96) -> (N,128) can be plugged in instead, or the batch may carry 'image_features'
        self.vision_encoder = vision_encoder
        self._vision_sd = vision_encoder_state_dict
        if vision_encoder_state_dict is not None:     # ... or a whole autoencoder checkpoint's state_dict (autoencoder.state_dict())
            from .vision import encoder_state_dict_from
            self._vision_sd = encoder_state_dict_from(vision_encoder_state_dict) or vision_encoder_state_dict
        # train_vision_encoder: the reference's behaviour -- its encoder is a registered submodule, so Adam(self.parameters())
        # (:115-116) optimises it with the U-Net.  Off (this project's default) the encoder stays frozen.
        self.train_vision_encoder = bool(train_vision_encoder)
        if self.train_vision_encoder and vision_encoder is not None and not hasattr(vision_encoder, "train_forward"):
            raise ValueError("train_vision_encoder=True trains the HIP encoder (vision.VisionEncoder): pass "
                             "vision_encoder_state_dict, not a callable")
        self.device = torch.device("cuda", device)
        self._device_index = device
        self._max_batch = max_batch
        self._engine: Optional[SpdmEngine] = None
        self._engine_key = None
        self._train_engine: Optional[SpdmEngine] = None     # training_step(backward=True): cached apart from sampling
        self._train_key = None
        self._ema = None                                    # configure_ema(): optim.DeviceEMA over the optimiser's parameters
        self._ema_swapped = False                           # inside ema_weights(): the engines hold the shadow

    # ------------------------------------------------------------------------------------------
    _HPARAM_KEYS = ("noise_steps", "obs_horizon", "pred_horizon", "observation_dim", "prediction_dim", "learning_rate",
                    "model", "noise_scheduler_type", "inpaint_horizon", "step_size")

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, hparams_file=None, map_location=None, use_ema: bool = False, **kwargs):
        """Lightning's ``LightningModule.load_from_checkpoint(ckpt, hparams_file=yaml)`` as generate.py:25,27 and
        run_predictions.py call it: constructor arguments from ``hparams.yaml`` (``save_hyperparameters()`` of
        models/diffusion_ddpm.py:37), U-Net tensors from the checkpoint's ``noise_estimator.*`` entries, the observation
        encoder's from its ``vision_encoder.*`` entries when present (vision.VisionEncoder).  ``use_ema=True``: the model's
        weights are the averaged tensors of the checkpoint's ``ema_state_dict`` instead (``save_checkpoint`` of a model with
        ``configure_ema()``) -- for inference; raises when the file holds none."""
        from .weights import check_state_dict, fetch_hyperparams_from_yaml, load_checkpoint_state_dict
        hp = dict(fetch_hyperparams_from_yaml(hparams_file)) if hparams_file else {}
        ctor = {k: hp[k] for k in cls._HPARAM_KEYS if k in hp}
        if isinstance(hp.get("vision_encoder"), str) or hp.get("vision_encoder") is None:
            pass                                   # a name (e.g. 'resnet18') in the yaml is not a callable: ignored
        ctor.update(kwargs)
        if use_ema:
            return cls._load_ema_checkpoint(str(checkpoint_path), ctor)
        sd, other = load_checkpoint_state_dict(str(checkpoint_path))
        model = ctor.get("model", "UNet")            # (no key: the constructor's default, simple_Unet.UNet)
        attention = model != "UNet_FilmnoAttention"
        cond_dim = int(ctor.get("observation_dim", 2)) * int(ctor.get("obs_horizon", 10))
        check_state_dict(sd, cond_dim, attention=attention, model=model, noise_steps=int(ctor.get("noise_steps", 1000)))
        if "vision_encoder_state_dict" not in ctor and any(k.startswith("vision_encoder.") for k in other):
            from .vision import encoder_state_dict_from
            from .weights import safe_load_state_dict
            ctor["vision_encoder_state_dict"] = encoder_state_dict_from(safe_load_state_dict(str(checkpoint_path)))
        return cls(state_dict=sd, **ctor)

    @classmethod
    def _load_ema_checkpoint(cls, checkpoint_path: str, ctor: dict):
        """``load_from_checkpoint(use_ema=True)``: the model built from ``ema_state_dict``'s tensors.  The encoder is the
        averaged one when the checkpoint averaged it, the checkpoint's own otherwise."""
        from .vision import encoder_state_dict_from
        from .weights import check_state_dict
        ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        ema_sd = ck.get("ema_state_dict") if isinstance(ck, dict) else None
        if not isinstance(ema_sd, dict) or not ema_sd:
            raise ValueError(f"{checkpoint_path} holds no 'ema_state_dict': it was written by a run without an EMA of the "
                             f"weights (train --ema, or configure_ema() before save_checkpoint); load it without use_ema")
        prefix = "noise_estimator."
        sd = {k[len(prefix):]: v for k, v in ema_sd.items() if k.startswith(prefix)}
        model = ctor.get("model", "UNet")
        cond_dim = int(ctor.get("observation_dim", 2)) * int(ctor.get("obs_horizon", 10))
        check_state_dict(sd, cond_dim, attention=model != "UNet_FilmnoAttention", model=model,
                         noise_steps=int(ctor.get("noise_steps", 1000)))
        if "vision_encoder_state_dict" not in ctor:
            enc = encoder_state_dict_from(ema_sd) or encoder_state_dict_from(ck.get("state_dict", {}))
            if enc is not None:
                ctor["vision_encoder_state_dict"] = enc
        return cls(state_dict=sd, **ctor)

    # Lightning look-alikes used by callers (generate.py:36)
    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    # ------------------------------------------------------------------------------------------
    def _engine_for(self, batch: int, H: int, D: int, pin: bool = False) -> SpdmEngine:
        spec = _as_spec(self.noise_scheduler)
        if self.simple:
            # simple_Unet.py: the time table is the network's own pos_encoding buffer (noise_steps + 1 rows at construction);
            # a schedule reaching past it is refused when it is installed, as the reference's pe[t] would fail
            T = int(self.noise_estimator._host_sd["pos_encoding.pos_encoding"].shape[0])      # (a shape: no refresh from the device)
        else:
            T = max(int(spec.config.num_train_timesteps), int(self.noise_steps))
        key = ("UNet" if self.simple else self.attention, H, D, T, batch if pin else 0)   # (a pinned engine: ONE global batch)
        if self._engine is None or self._engine_key != key or batch > self._engine.max_batch:
            if self._engine is not None:
                self._engine.close()
            self._engine = SpdmEngine(H, D, self.cond_dim, max_batch=batch if pin else max(batch, self._max_batch),
                                      device=self._device_index, attention=self.attention,
                                      num_train_timesteps=T, pin_geometry=pin,
                                      model="UNet" if self.simple else None)
            self._engine.load_state_dict(self.noise_estimator._sd)
            self._engine_key = key
            if self._ema_swapped:           # built inside ema_weights(): it takes the shadow like the engines swapped on entry
                self.noise_estimator._push(self._ema.shadow[0], engines=[self._engine])
        return self._engine

    def _check_trainable(self) -> None:
        if self.attention and not self.train_attention:
            raise NotImplementedError(
                f"training_step(backward=True) computes gradients for model='UNet_FilmnoAttention', for simple_Unet.py's "
                f"model='UNet', or for model='UNet_Film' constructed with train_attention=True (this model is "
                f"{self.model_name!r})")

    def _train_engine_for(self, batch: int, H: int, D: int) -> SpdmEngine:
        self._check_trainable()
        if self.simple:      # simple_Unet.py: the time table is the network's own pos_encoding buffer (as in _engine_for)
            T = int(self.noise_estimator._host_sd["pos_encoding.pos_encoding"].shape[0])      # (a shape: no refresh from the device)
        else:
            T = max(int(_as_spec(self.noise_scheduler).config.num_train_timesteps), int(self.noise_steps))
        key = (H, D, T)
        if self._train_engine is None or self._train_key != key or batch > self._train_engine.max_batch:
            if self._train_engine is not None:
                self._train_engine.close()
            self._train_engine = SpdmEngine(H, D, self.cond_dim, max_batch=max(batch, self._max_batch),
                                            device=self._device_index, attention=self.attention, num_train_timesteps=T,
                                            train=True, train_attention=self.attention and not self.simple,
                                            model="UNet" if self.simple else None, train_simple=self.simple)
            self._train_engine.load_state_dict(self.noise_estimator._sd)
            self._train_key = key
            if self._ema_swapped:
                self.noise_estimator._push(self._ema.shadow[0], engines=[self._train_engine])
        return self._train_engine

    def add_constraints(self, x_t: torch.Tensor, x_inpaint: torch.Tensor) -> torch.Tensor:
        """models/diffusion_ddpm.py:216-219 (in place, broadcast over the batch)."""
        x_t[:, :, :self.inpaint_horizon, :] = x_inpaint
        return x_t

    # ==================== Sampling (models/diffusion_ddpm.py:223-277) ====================
    def sample(self, batch: Dict[str, torch.Tensor], option: Optional[str] = None, *,
               x_T: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
               batched: bool = False, seed: Optional[int] = None, sample_offset: int = 0, every: int = 1,
               sharded: Optional[bool] = None, group=None, shard_exact: bool = False, candidates: int = 1, use_ema: bool = False,
               start_step: int = 0):
        """``option``: None -> x_0 (B,1,H,D); 'sample_history' -> list of the N+1 iterates (the reference's form);
        'sample_history_stream' -> a generator of ``(i, x_i)`` host tensors handed out while the loop runs
        (``every``: stride in steps; SpdmEngine.sample_stream).

        ``seed``: key of the device noise stream that replaces the ``torch.randn`` diffusers' DDPM ``step`` draws from
        the global generator on every step of every call.  None (default) draws a FRESH 62-bit seed per call from
        torch's global generator -- so, as with the reference, two calls give different trajectories and
        ``torch.manual_seed`` makes a run reproducible.  Ignored when ``noise`` is supplied.

        ``sharded`` (with ``batched=True``): every rank of the process group passes the SAME global batch; each runs its
        contiguous slice of the trajectories on its own GPU (no communication inside the loop) and one all-gather -- RCCL
        over xGMI on the "nccl" backend -- returns all B trajectories on every rank, rank-major, independent of the rank
        count (distributed.ShardedSampler).  None (default): shard iff a process group with more than one rank is
        initialised.  ``x_T`` and ``seed`` left at None are drawn on rank 0 and broadcast.  A shard's trajectories agree
        with the single-GPU run to fp32 rounding (<= 1e-5 over a loop: a small shard selects other kernels for the coarse
        levels); ``shard_exact=True`` pins every rank's kernel selection to that of the GLOBAL batch instead -- bit-identical
        to the single-GPU run, at the price of small-batch kernels not being used on small shards.

        ``start_step = i0 > 0`` runs a suffix of the loop: ``x_T``, then required, is the iterate the loop
        has after ``i0`` of its ``noise_steps`` iterations, and only iterations ``[i0, noise_steps)`` run -- bit for bit the
        tail of the whole loop from that iterate under DDPM / DDIM.  Under ``DPMSolverMultistepScheduler`` a suffix is a new
        session and begins with a first-order step (no previous x_0 exists), so it is NOT the whole loop's tail (DESIGN.md
        8.19).  Not available with a history option or ``sharded=True``.

        ``candidates = K > 1`` (with ``batched=True``) samples K trajectories per row of the batch: ``obs_cond``
        and ``inpaint`` are built for the E rows -- the frame encoder runs E obs_h frames -- and each row is then repeated K
        times on the device, so row ``e K + k`` of the (E K,1,H,D) result is candidate k of row e.  ``x_T``, if given, is
        (E K,1,H,D).  The device noise is keyed by the row index, so every candidate has a stream of its own.  Not available
        with a history option or ``sharded=True``.

        ``use_ema=True`` runs the call inside ``ema_weights()``: the engines hold the averaged weights for
        its duration.  It raises when no EMA is configured, and with ``option='sample_history_stream'``, whose generator
        would run after the live weights are back."""
        if use_ema:
            if option == "sample_history_stream":
                raise ValueError("use_ema=True is not available with option='sample_history_stream': the generator runs after "
                                 "this call has put the live weights back")
            with self.ema_weights():
                return self.sample(batch, option, x_T=x_T, noise=noise, batched=batched, seed=seed, sample_offset=sample_offset,
                                   every=every, sharded=sharded, group=group, shard_exact=shard_exact, candidates=candidates,
                                   start_step=start_step)
        from .distributed import ShardedSampler, shard_bounds, world_and_rank
        if isinstance(candidates, bool) or not isinstance(candidates, (int, np.integer)) or candidates < 1:
            raise ValueError(f"candidates = {candidates!r} must be an integer >= 1")
        candidates = int(candidates)
        if isinstance(start_step, bool) or not isinstance(start_step, (int, np.integer)) or not 0 <= start_step < int(self.noise_steps):
            raise ValueError(f"start_step = {start_step!r} must be an integer in [0, noise_steps = {self.noise_steps})")
        start_step = int(start_step)
        if start_step and x_T is None:
            raise ValueError("start_step > 0 needs x_T: the iterate the loop has after start_step steps")
        world, rank = world_and_rank(group)
        if sharded is None:
            sharded = batched and world > 1
        if start_step and (option in ("sample_history", "sample_history_stream") or sharded):
            raise ValueError("start_step > 0 runs a suffix of the loop on this process: not available with option='sample_history', "
                             "'sample_history_stream' or sharded=True")
        if candidates > 1 and (not batched or sharded or option in ("sample_history", "sample_history_stream")):
            raise ValueError("candidates > 1 repeats the rows of a batch on this process: it needs batched=True and is not available "
                             "with sharded=True, option='sample_history' or 'sample_history_stream'")
        if sharded and not batched:
            raise ValueError("sharded=True needs batched=True (the reference's B = 1 form has nothing to shard)")
        if sharded and option == "sample_history_stream":
            raise ValueError("option='sample_history_stream' hands out this process's iterates: not available with sharded=True")
        if seed is None:
            seed_t = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)
            if sharded and world > 1:
                seed_t = self._broadcast0(seed_t, group)
            seed = int(seed_t.item())
        for key, tensor in batch.items():
            batch[key] = tensor.to(self.device)
        obs_cond = self.prepare_obs_cond_vectors(batch)                       # (B, obs_h, obs_dim)
        inpaint = self.prepare_inpaint_vectors(batch)                         # (B, inp_h, pred_dim)
        if not batched:                                                       # reference: B forced to 1
            obs_cond, inpaint = obs_cond[0:1], inpaint[0:1]
        obs_cond = obs_cond.unsqueeze(1)                                      # (B,1,obs_h,obs_dim)
        inpaint = inpaint.unsqueeze(1)                                        # (B,1,inp_h,pred_dim)
        H, D = self.pred_horizon + self.inpaint_horizon, self.prediction_dim
        if candidates > 1:                                                    # 1: exactly the call without the keyword
            obs_cond = obs_cond.repeat_interleave(candidates, dim=0)          # row e K + k is row e
            inpaint = inpaint.repeat_interleave(candidates, dim=0)
            if x_T is not None and tuple(x_T.shape) != (obs_cond.shape[0], 1, H, D):
                raise ValueError(f"x_T must be {(obs_cond.shape[0], 1, H, D)} with candidates = {candidates}, got {tuple(x_T.shape)}")
        B = obs_cond.shape[0]
        if x_T is None:
            x_T = torch.rand(B, 1, H, D, device=self.device)                  # uniform, :252
            if sharded and world > 1:
                x_T = self._broadcast0(x_T, group)
        spec = _as_spec(self.noise_scheduler)
        spec.set_timesteps(self.noise_steps)                                  # :257/:268
        s0, s1 = shard_bounds(B, rank, world) if sharded else (0, B)
        eng = self._engine_for(B if (sharded and shard_exact) else s1 - s0, H, D, pin=bool(sharded and shard_exact))
        eng.set_scheduler(spec)
        ip = inpaint if self.inpaint_horizon > 0 else None
        if option == "sample_history_stream":
            return eng.sample_stream(obs_cond, x_T, noise=noise, inpaint=ip, seed=seed, sample_offset=sample_offset, every=every)
        want_hist = (option == "sample_history")
        if sharded:
            if sample_offset:
                raise ValueError("sample_offset is the shard's own bookkeeping when sharded=True")
            res = ShardedSampler(eng, group).sample(obs_cond, x_T, noise=noise, inpaint=ip, seed=seed, history=want_hist)
        else:
            extra = {"start_step": start_step} if start_step else {}              # 0: exactly the call without the keyword
            res = eng.sample(obs_cond, x_T, noise=noise, inpaint=ip, seed=seed, sample_offset=sample_offset, history=want_hist, **extra)
        if want_hist:
            _, hist = res
            return [hist[i] for i in range(hist.shape[0])]                    # list of N+1 (B,1,H,D), :256-265
        return res

    def _broadcast0(self, t: torch.Tensor, group=None) -> torch.Tensor:
        """rank 0's value of ``t`` on every rank (through the device for a backend that only moves device tensors)."""
        import torch.distributed as dist
        dev = self.device if dist.get_backend(group) == "nccl" else torch.device("cpu")
        buf = t.to(dev).contiguous()
        dist.broadcast(buf, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return buf.to(t.device)

    # ==================== Helper functions (models/diffusion_ddpm.py:283-348) ====================
    def prepare_observation_batch(self, batch):
        out = {}
        for k in ("image", "position", "action", "velocity", "image_features"):
            if k in batch:
                out[k] = batch[k][:, :self.obs_horizon].to(self.device).float()
        return out

    def prepare_obs_cond_vectors(self, observation_batch):
        if "obs_cond" in observation_batch:
            return observation_batch["obs_cond"].float()
        if "image_features" in observation_batch:
            feats = observation_batch["image_features"]
        else:
            if self.vision_encoder is None and self._vision_sd is not None:
                from .vision import VisionEncoder
                self.vision_encoder = VisionEncoder(self._vision_sd, device=self._device_index)
            if self.vision_encoder is None:
                raise RuntimeError("batch has raw images but neither vision_encoder nor vision_encoder_state_dict was "
                                   "supplied (the reference's autoencoder checkpoint is not part of the repo)")
            img = observation_batch["image"]
            with torch.no_grad():
                enc = self.vision_encoder(img.flatten(end_dim=1))
            feats = enc.reshape(*img.shape[:2], -1)
        return torch.cat([observation_batch["position"], observation_batch["action"],
                          observation_batch["velocity"], feats], dim=-1)

    def _trained_obs_cond_vectors(self, observation_batch):
        """``prepare_obs_cond_vectors`` as the reference's ``training_step`` runs it, the encoder recorded for the backward
        pass (``VisionEncoder.train_forward``).  Only raw frames can be differentiated through."""
        if "image" not in observation_batch or "image_features" in observation_batch or "obs_cond" in observation_batch:
            raise ValueError("train_vision_encoder=True needs raw 'image' frames in the batch (and no precomputed "
                             "'image_features' / 'obs_cond'): there is nothing else to differentiate")
        img = observation_batch["image"]
        enc = self._trainable_encoder().train_forward(img.flatten(end_dim=1))
        feats = enc.reshape(*img.shape[:2], -1)
        return torch.cat([observation_batch["position"], observation_batch["action"],
                          observation_batch["velocity"], feats], dim=-1)

    def prepare_inpaint_vectors(self, observation_batch):
        if "inpaint" in observation_batch:
            return observation_batch["inpaint"].float()
        if self.inpaint_horizon == 0:
            B = next(iter(observation_batch.values())).shape[0]
            return torch.zeros(B, 0, self.prediction_dim, device=self.device)
        pos = observation_batch["position"][:, -self.inpaint_horizon:, :]
        act = observation_batch["action"][:, -self.inpaint_horizon:, :]
        return torch.cat([pos, act], dim=-1)

    def prepare_prediction_batch(self, batch):
        """models/diffusion_ddpm.py:300-315: everything after the observed window, ``batch[k][:, self.obs_horizon:]``
        (the dataset windows are obs_horizon + pred_horizon long, so this is the last pred_horizon entries)."""
        out = {}
        for k in ("image", "position", "action", "velocity", "image_features"):
            if k in batch:
                out[k] = batch[k][:, self.obs_horizon:].to(self.device).float()
        return out

    def prepare_prediction_vectors(self, prediction_batch):
        """models/diffusion_ddpm.py:332-338: x_0 = cat(position, action)."""
        return torch.cat([prediction_batch["position"], prediction_batch["action"]], dim=-1)

    # ==================== Validation (models/diffusion_ddpm.py:175-214) ====================
    def validate(self, batch, *, x_T: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None):
        """The reference's validation sampler: the first trajectory of the batch through the full loop; returns
        ``(x_0 (1,1,H,D), observation_batch, inpaint_vector (1,1,inp_h,D))``."""
        observation_batch = self.prepare_observation_batch(batch)
        inpaint_vector = self.prepare_inpaint_vectors(observation_batch)[0:1].unsqueeze(1)
        x_0 = self.sample(dict(observation_batch), x_T=x_T, noise=noise)
        return x_0, observation_batch, inpaint_vector

    # ==================== Training (models/diffusion_ddpm.py:128-173) ====================
    def forward_process(self, prediction_vector: torch.Tensor, x_0_inpaint: Optional[torch.Tensor], **kw):
        """``noising.forward_process`` with this model's scheduler tables: timesteps, noise, ``add_noise`` and
        ``add_constraints`` (and, with ``time_dim`` / ``dropout_p``, the time-embedding dropout mask) in one HIP launch.
        The tables are cached per scheduler OBJECT and device: assign a new ``noise_scheduler`` rather than editing one's
        ``config`` in place.  Returns ``(x_noisy, noise, t[, time_scale])`` on the device; keywords as there (``t``, ``noise``, ``seed``, ``step``,
        ``sample_offset``, ``time_dim``, ``dropout_p``)."""
        from .noising import forward_process
        if self._fp_spec[0] is not self.noise_scheduler:   # a diffusers-like scheduler is restated once per object, not per
            self._fp_spec = (self.noise_scheduler, _as_spec(self.noise_scheduler))      # call: the device tables stay cached
        sa, sb = self._fp_spec[1].device_tables(prediction_vector.device)
        T = min(int(self.noise_steps), sa.numel())         # the reference draws t in [0, noise_steps)
        return forward_process(prediction_vector, x_0_inpaint, sa[:T], sb[:T], **kw)

    def training_step(self, batch, batch_idx: int = 0, *, t: Optional[torch.Tensor] = None,
                      noise: Optional[torch.Tensor] = None, return_parts: bool = False, backward: bool = False,
                      time_scale: Optional[torch.Tensor] = None, device_noise: bool = False, seed: int = 0,
                      noise_step: Optional[int] = None, sample_offset: int = 0, time_dropout: Optional[float] = None):
        """The reference's ``training_step``: noising of the target window at a per-sample timestep (``add_noise``),
        in-painting of the observed rows, ONE U-Net evaluation with ``t`` of shape (B,), MSE against the noise.  The U-Net
        runs on the HIP path (``spdm_unet_forward`` with per-sample t); the returned loss carries no torch graph.
        ``backward=True`` (model='UNet_FilmnoAttention', 'UNet', or 'UNet_Film' with ``train_attention=True``;
        NotImplementedError otherwise) is ``loss.backward()`` as
        well: the step runs ``spdm_train_loss_grad`` on a training engine cached apart from the sampling engines and
        leaves the gradients in ``noise_estimator.grads()`` (and d loss / d obs_cond in ``noise_estimator.grad_cond``)
        for a torch optimiser; ``noise_estimator.load_state_dict`` takes the updated weights back.
        ``t`` / ``noise`` may be passed for reproducibility (the reference draws them with torch.randint / randn_like).
        ``time_scale`` (model='UNet' with ``backward=True`` only; ValueError otherwise): the (B, time_dim) multiplier of
        pe[t] that PositionalEncoding's Dropout(p=0.1) applies in training mode.  The caller draws it as the reference's
        dropout would: ``F.dropout(torch.ones(B, 256, device='cuda'), 0.1, True)``.  Without it the step is the eval-mode
        network's (no dropout).
        ``device_noise=True``: timesteps, noise, ``add_noise`` and ``add_constraints`` are ONE HIP launch
        (``forward_process``) instead of torch's global RNG and a dozen small launches, and ``t`` reaches the
        engine as a device tensor: with ``backward=True`` the step then runs no torch-side ``.cpu()`` of ``t`` and no host
        range check (the library's own waits inside the training pass remain).  The randomness is a pure function of ``(seed, noise_step, sample_offset + b)``; ``noise_step=None``
        takes a counter of this object that advances by one per such call; a rank of a sharded batch passes
        ``sample_offset = rank * B`` (distributed.py's convention).  ``t`` / ``noise`` are still honoured.
        ``time_dropout=p`` (with ``device_noise=True``, model='UNet' and ``backward=True`` only; ValueError otherwise, and
        with ``time_scale`` as well): the dropout mask is drawn in the same launch and used as ``time_scale``."""
        if time_scale is not None and not (backward and self.simple):
            raise ValueError("time_scale applies to model='UNet' (simple_Unet.py's dropout on pe[t]) with backward=True only")
        if time_dropout is not None:
            if time_scale is not None:
                raise ValueError("pass time_scale (a drawn mask) or time_dropout (a probability), not both")
            if not (backward and self.simple):
                raise ValueError("time_dropout applies to model='UNet' (simple_Unet.py's dropout on pe[t]) with backward=True only")
            if not device_noise:
                raise ValueError("time_dropout draws its mask in the device forward process: it needs device_noise=True")
            if not 0.0 <= float(time_dropout) < 1.0:
                raise ValueError(f"time_dropout must be a probability in [0, 1), got {time_dropout}")
        if backward:
            self._check_trainable()
        observation_batch = self.prepare_observation_batch(batch)
        prediction_batch = self.prepare_prediction_batch(batch)
        joint = backward and self.train_vision_encoder
        if joint:
            obs_cond = self._trained_obs_cond_vectors(observation_batch).unsqueeze(1)
        else:
            obs_cond = self.prepare_obs_cond_vectors(observation_batch).unsqueeze(1)        # (B,1,obs_h,obs_dim)
        x_0 = self.prepare_prediction_vectors(prediction_batch).unsqueeze(1)               # (B,1,pred_h,pred_dim)
        x_0_inpaint = self.prepare_inpaint_vectors(observation_batch).unsqueeze(1)         # (B,1,inp_h,pred_dim)
        B = x_0.shape[0]
        if device_noise:
            prediction_vector = torch.cat([x_0_inpaint, x_0], dim=2)                       # concat in time
            if noise_step is None:
                noise_step, self._noise_step = self._noise_step, self._noise_step + 1
            kw = dict(t=t, noise=noise, seed=seed, step=noise_step, sample_offset=sample_offset)
            if time_dropout is not None:
                eng = self._train_engine_for(B, prediction_vector.shape[-2], prediction_vector.shape[-1])
                kw.update(time_dim=eng.time_dim, dropout_p=float(time_dropout))
            out = self.forward_process(prediction_vector, x_0_inpaint, **kw)
            x_noisy, noise, t = out[:3]                                                    # t: device int32
            if time_dropout is not None:
                time_scale = out[3]
            if not backward:
                t = t.long()
        else:
            if t is None:
                t = torch.randint(0, self.noise_steps, (B,), device=self.device)
            t = t.to(self.device).long()
            prediction_vector = torch.cat([x_0_inpaint, x_0], dim=2)                       # concat in time
            if noise is None:
                noise = torch.randn_like(prediction_vector)
            noise = noise.to(self.device).float()
            x_noisy = _as_spec(self.noise_scheduler).add_noise(prediction_vector, noise, t)
            x_noisy = self.add_constraints(x_noisy, x_0_inpaint)
        if backward:
            eng = self._train_engine_for(B, x_noisy.shape[-2], x_noisy.shape[-1])
            loss, noise_estimated, g, grad_cond = eng.loss_and_grad(x_noisy, t, obs_cond, noise, flat=True, time_scale=time_scale)
            grads = {}
            for name, off, shape in eng._index:
                if self.simple and name == "pos_encoding.pos_encoding":      # a buffer, not a parameter
                    continue
                n = int(np.prod(shape)) if shape else 1
                grads[name] = g[off:off + n].view(shape)
            ne = self.noise_estimator
            if ne._flat is not None and ne._flat_index == eng._index:
                ne._flat.grad = g                 # loss.backward(): the flat gradient, the same storage as grads()
            self.noise_estimator._grads = grads
            self.noise_estimator.grad_cond = grad_cond
            if joint:       # d loss / d latents = the feature columns of d loss / d obs_cond; gradients in vision_encoder.grads()
                from .vision import feature_grad
                self.vision_encoder.backward(feature_grad(grad_cond, obs_cond.shape[-2], obs_cond.shape[-1]))
            return (loss, noise_estimated, x_noisy) if return_parts else loss
        noise_estimated = self.noise_estimator(x_noisy, t, obs_cond)
        loss = torch.mean((noise - noise_estimated) ** 2)                                  # nn.MSELoss, :49
        return (loss, noise_estimated, x_noisy) if return_parts else loss

    def validation_step(self, batch, batch_idx: int = 0, **kw):
        return self.training_step(batch, batch_idx, **kw)

    def validation_loss(self, batches, *, seed: int = 0, noise_step: int = 0xFFFFFFFF, return_terms: bool = False,
                        use_ema: bool = False):
        """The reference's ``val_loss`` (``validation_step`` over a ``val_dataloader()``, averaged by Lightning over the epoch
        with batch-size weights) as a deterministic function of the weights, formed on the device.

        Every batch of ``batches`` goes through ONE ``forward_process`` keyed by ``(seed, noise_step, sample_offset = the
        number of validation samples before the batch)`` -- so a sample's noise and timestep depend on its position in the
        validation order, not on the batch size or on how often validation runs; ``noise_step`` is a value no training step
        uses -- then through the forward-only engine with ``t`` left on the device (``spdm_unet_forward_dt``; for
        model='UNet' the eval-mode network, no dropout) and through ``spdm_loss_terms``, which writes each sample's mean
        squared error to its slot of a float64 buffer.  After the last batch one ``spdm_eval_reduce`` takes the mean and ONE
        read-back returns it as a Python float: every element weighs equally.  ``return_terms=True``: ``(val_loss, terms (N)
        float64, t (N) int32)``, the last two on the device.  Forward-only: it serves all three models, ``'UNet_Film'``
        without ``train_attention`` included.  ``use_ema=True``: the same pass with the averaged weights in
        the engines (``ema_weights()``); raises when no EMA is configured."""
        if use_ema:
            with self.ema_weights():
                return self.validation_loss(batches, seed=seed, noise_step=noise_step, return_terms=return_terms)
        from .evaluation import reduce_errors
        from .train_metrics import loss_terms_into
        ids = getattr(batches, "window_ids", None)
        cap = len(ids) if ids is not None else 1024
        terms = torch.empty(max(cap, 1), dtype=torch.float64, device=self.device)
        slot_t = torch.empty(max(cap, 1), dtype=torch.int32, device=self.device)
        count = 0
        for batch in batches:
            observation_batch = self.prepare_observation_batch(batch)
            prediction_batch = self.prepare_prediction_batch(batch)
            obs_cond = self.prepare_obs_cond_vectors(observation_batch).unsqueeze(1)
            x_0 = self.prepare_prediction_vectors(prediction_batch).unsqueeze(1)
            x_0_inpaint = self.prepare_inpaint_vectors(observation_batch).unsqueeze(1)
            prediction_vector = torch.cat([x_0_inpaint, x_0], dim=2)
            B = prediction_vector.shape[0]
            if count + B > terms.numel():       # a source of unknown length: the buffers grow on the device
                grow = max(terms.numel(), count + B - terms.numel())
                terms = torch.cat([terms, torch.empty(grow, dtype=torch.float64, device=self.device)])
                slot_t = torch.cat([slot_t, torch.empty(grow, dtype=torch.int32, device=self.device)])
            x_noisy, noise, t = self.forward_process(prediction_vector, x_0_inpaint, seed=seed, step=noise_step, sample_offset=count)
            eng = self._engine_for(B, x_noisy.shape[-2], x_noisy.shape[-1])
            eps = eng.unet_forward(x_noisy, t, obs_cond)
            loss_terms_into(eps, noise, terms, count, t=t, slot_t=slot_t)
            count += B
        if count == 0:
            raise ValueError("validation_loss: no batches")
        terms, slot_t = terms[:count], slot_t[:count]
        mean = reduce_errors(terms.view(count, 1), 1)[2]
        val_loss = float(mean.item())           # the one read-back
        return (val_loss, terms, slot_t) if return_terms else val_loss

    # ==================== Checkpoints (Lightning's layout; train.py's ModelCheckpoint) ====================
    def hparams(self) -> dict:
        """The constructor arguments ``save_hyperparameters()`` records (models/diffusion_ddpm.py:37)."""
        hp = {"noise_steps": self.noise_steps, "obs_horizon": self.obs_horizon, "pred_horizon": self.pred_horizon,
              "observation_dim": self.observation_dim, "prediction_dim": self.prediction_dim, "learning_rate": self.lr,
              "model": self.model_name, "noise_scheduler_type": self.noise_scheduler_type,
              "inpaint_horizon": self.inpaint_horizon, "step_size": self.step_size}
        hp = {k: (v.item() if hasattr(v, "item") else v) for k, v in hp.items()}
        assert tuple(hp) == self._HPARAM_KEYS
        hp["vision_encoder"] = None
        return hp

    def save_hparams(self, path) -> None:
        """The ``hparams.yaml`` that ``load_from_checkpoint(hparams_file=)`` reads."""
        import yaml
        with open(path, "w") as fh:
            fh.write(yaml.safe_dump(self.hparams(), sort_keys=False))

    def save_checkpoint(self, path, *, optimizer=None, scheduler=None, trainer_state: Optional[dict] = None) -> None:
        """Write ``path`` with ``torch.save`` in the layout of a Lightning checkpoint: ``state_dict`` (``noise_estimator.<name>``
        for every tensor of the network at its CURRENT value -- pulled from the flat device parameter if an optimiser has
        moved it -- the ``pos_encoding.pos_encoding`` buffer of model='UNet' included, and ``vision_encoder.<name>`` when the
        model has encoder weights), ``hyper_parameters``, ``epoch``, ``global_step``, ``optimizer_states``, ``lr_schedulers``,
        and this project's own counters under ``'spdm_trainer'`` (``trainer_state``; ``epoch`` and ``global_step`` are taken
        from it).  Tensors are saved from the host; the file holds nothing ``torch.load(weights_only=True)`` refuses."""
        def host(v):
            if isinstance(v, torch.Tensor):
                return v.detach().cpu()
            if isinstance(v, dict):
                return {k: host(x) for k, x in v.items()}
            if isinstance(v, (list, tuple)):
                return [host(x) for x in v]
            if isinstance(v, np.generic):
                return v.item()
            return v

        self.noise_estimator.mark_moved()       # whoever stepped the flat parameter, and however: the file holds its values
        sd = {"noise_estimator." + k: v.clone() for k, v in self.noise_estimator.state_dict().items()}
        enc = None
        if hasattr(self.vision_encoder, "state_dict"):
            enc = self.vision_encoder.state_dict()
        elif self._vision_sd is not None:
            enc = self._vision_sd
        for k, v in (enc or {}).items():
            sd["vision_encoder." + k] = v.detach().cpu().clone() if hasattr(v, "detach") else torch.from_numpy(np.array(v))
        ts = host(dict(trainer_state or {}))
        ckpt = {"epoch": int(ts.get("epoch", 0)), "global_step": int(ts.get("global_step", 0)),
                "pytorch-lightning_version": "2.0.0",
                "state_dict": sd, "hyper_parameters": self.hparams(),
                "optimizer_states": [host(optimizer.state_dict())] if optimizer is not None else [],
                "lr_schedulers": [host(scheduler.state_dict())] if scheduler is not None else [],
                "spdm_trainer": ts}
        if self._ema is not None:               # (no EMA: the file is what it was, key for key)
            ckpt["ema_state_dict"] = self._ema_host_state_dict()
            ckpt["spdm_ema"] = {"optimization_step": int(self._ema.optimization_step), "schedule": dict(self._ema.schedule)}
        torch.save(ckpt, str(path))

    def _ema_host_state_dict(self) -> Dict[str, torch.Tensor]:
        """The shadow as host tensors under checkpoint names: ``noise_estimator.<name>``, and ``vision_encoder.<name>`` when
        the encoder is averaged."""
        out = {"noise_estimator." + k: torch.from_numpy(v) for k, v in self.noise_estimator._unpack(self._ema.shadow[0]).items()}
        if len(self._ema.shadow) > 1:
            host = self._ema.shadow[1].detach().cpu()
            for name, off, shape in self.vision_encoder._index:
                out["vision_encoder." + name] = host[off:off + int(torch.Size(shape).numel())].reshape(shape).clone()
        return out

    def restore_checkpoint(self, ckpt: dict) -> None:
        """Take the ``noise_estimator.*`` tensors of a loaded checkpoint dict (``train.fit(ckpt_path=)``): host copy, flat
        parameter and every cached engine follow.  A jointly trained encoder is not restored here."""
        if self.train_vision_encoder:
            raise NotImplementedError("resuming a run with train_vision_encoder=True is not supported: the encoder's "
                                      "weights would not be restored")
        sd = {k[len("noise_estimator."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("noise_estimator.")}
        if not sd:
            raise ValueError("the checkpoint's state_dict holds no noise_estimator.* tensors")
        self.noise_estimator.load_state_dict(sd)
        if self._ema is not None:               # configure_ema() came first: its shadow and counter are the checkpoint's
            ema_sd, meta = ckpt.get("ema_state_dict"), ckpt.get("spdm_ema")
            if not ema_sd or not isinstance(meta, dict):
                raise ValueError("an EMA is configured but the checkpoint holds no 'ema_state_dict' / 'spdm_ema': it was "
                                 "written by a run without one")
            blob, idx = pack_state_dict(state_dict_to_numpy(
                {k[len("noise_estimator."):]: v for k, v in ema_sd.items() if k.startswith("noise_estimator.")}))
            if _index_of(idx) != self.noise_estimator._flat_index:
                raise ValueError("the checkpoint's ema_state_dict does not pack into this model's weight layout")
            self._ema.load_state_dict({"shadow": [torch.from_numpy(blob)], "optimization_step": meta["optimization_step"],
                                       "schedule": meta["schedule"]})

    # ==================== Optimisation (models/diffusion_ddpm.py:114-124, train.py) ====================
    def configure_optimizers(self, device_optimizer: bool = False):
        """The reference's optimiser: Adam(lr) over the weights -- here the one flat device parameter
        (``noise_estimator.flat_parameter()``) -- and ReduceLROnPlateau('min', patience=5) on ``val_loss``, in
        Lightning's dict shape.  ``device_optimizer=True``: the same dict with ``optim.DeviceAdam`` (clip + Adam in HIP,
        DESIGN.md 8.8) over the same parameters in torch.optim.Adam's place; its state dicts load into Adam and back."""
        params = [self.noise_estimator.flat_parameter()]
        if self.train_vision_encoder:       # Adam is elementwise: one Adam over both flat parameters == Adam(self.parameters())
            params.append(self._trainable_encoder().flat_parameter())
        if device_optimizer:
            from .optim import DeviceAdam
            optimizer = DeviceAdam(params, lr=self.lr)
        else:
            optimizer = torch.optim.Adam(params, lr=self.lr)
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, "min", patience=5)
        return {
            "optimizer": optimizer,
            "lr_scheduler": {
                "scheduler": scheduler,
                "monitor": "val_loss",
                "frequency": 1
            },
        }

    def optimizer_step(self, optimizer, gradient_clip_val: Optional[float] = 0.5) -> None:
        """One optimiser step after ``training_step(backward=True)``: clip the global gradient norm (Lightning's
        ``gradient_clip_val``, 0.5 in train.py), ``optimizer.step()``, then put the new weights into every cached engine
        in place (``SpdmEngine.update_weights``) -- no host round trip of the weights."""
        from .optim import DeviceAdam
        if self._ema_swapped:
            raise RuntimeError("optimizer_step inside ema_weights(): the engines hold the averaged weights")
        if isinstance(optimizer, DeviceAdam):       # clip (over all its parameters together) + Adam in two HIP launches
            optimizer.step(max_norm=gradient_clip_val or None)
            self.noise_estimator.mark_moved()
            self.noise_estimator._push()
            if self.train_vision_encoder:
                self.vision_encoder.update_weights(self._trainable_encoder().flat_parameter().detach())
            if self._ema is not None:       # the weights have moved: one more launch
                self._ema.step()
            return
        params = [self.noise_estimator.flat_parameter()]
        if self.train_vision_encoder:       # Lightning clips the norm over ALL parameters together
            params.append(self._trainable_encoder().flat_parameter())
        if gradient_clip_val:
            torch.nn.utils.clip_grad_norm_(params, gradient_clip_val)
        optimizer.step()
        self.noise_estimator._push()
        if self.train_vision_encoder:
            self.vision_encoder.update_weights(params[1].detach())
        if self._ema is not None:
            self._ema.step()

    # ==================== EMA of the weights ====================
    def configure_ema(self, **schedule):
        """Keep an exponential moving average of the weights from now on: an ``optim.DeviceEMA`` over exactly the parameters
        ``configure_optimizers`` hands the optimiser -- ``noise_estimator.flat_parameter()``, and the encoder's flat parameter
        with ``train_vision_encoder=True`` -- so it averages what the reference's ``Adam(self.parameters())`` steps.
        ``schedule``: ``optim.ema_decay``'s keywords.  ``optimizer_step`` updates it after the weights have moved;
        ``ema_weights()``, ``validation_loss(use_ema=True)`` and ``sample(use_ema=True)`` evaluate with it; ``save_checkpoint``
        writes it.  Stored on the model and returned."""
        from .optim import DeviceEMA
        if self._ema_swapped:
            raise RuntimeError("configure_ema inside ema_weights()")
        params = [self.noise_estimator.flat_parameter()]
        if self.train_vision_encoder:
            params.append(self._trainable_encoder().flat_parameter())
        self._ema = DeviceEMA(params, **schedule)
        return self._ema

    @contextlib.contextmanager
    def ema_weights(self):
        """``with model.ema_weights():`` -- every cached engine (and the encoder's handle, when it is averaged) holds the
        shadow inside the block and the live flat parameters again after it, also when the block raises.  The swap is
        ``SpdmEngine.update_weights`` in place, through ``NoiseEstimator._push``'s layout check and ``refresh_weights``
        fallback: no second handle, no host copy of the weights, the engines' addresses -- and a captured step graph -- stay
        valid.  An engine built inside the block takes the shadow too.  The flat parameters themselves are never written, so
        ``noise_estimator.state_dict()`` returns the live weights inside the block as outside.  Nesting raises."""
        if self._ema is None:
            raise RuntimeError("no EMA is configured: call configure_ema() (train --ema) first")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() is not re-entrant: the engines already hold the averaged weights")
        shadow = self._ema.shadow
        self._ema_swapped = True
        try:
            self.noise_estimator._push(shadow[0])
            if len(shadow) > 1:
                self.vision_encoder.update_weights(shadow[1], follow=False)
            yield self._ema
        finally:
            self._ema_swapped = False
            self.noise_estimator._push()
            if len(shadow) > 1:
                self.vision_encoder.update_weights(self._ema.params[1].detach())

    def _trainable_encoder(self):
        if self.vision_encoder is None:
            if self._vision_sd is None:
                raise RuntimeError("train_vision_encoder=True needs vision_encoder_state_dict")
            from .vision import VisionEncoder
            self.vision_encoder = VisionEncoder(self._vision_sd, device=self._device_index)
        return self.vision_encoder


class Diffusion_DDIM(Diffusion_DDPM):
    """models/diffusion_ddim.py:19-74: a byte-identical copy of the DDPM loop; it becomes DDIM only
    because the caller swaps ``noise_scheduler`` (generate.py:28-35).  Nothing to override here."""
    pass


def load_model(model_name: str, checkpoint_path=None, hparams_path=None, num_of_ddim_steps: int = 100, *,
               state_dict=None, solver_steps: Optional[int] = None, use_ema: bool = False, **hparams):
    """generate.py:23-37: build the sampler from a checkpoint + hparams.yaml (same positional signature as the
    reference) -- or from an in-memory ``state_dict`` / random init when no checkpoint is given -- and, for DDIM,
    overwrite scheduler and noise_steps exactly as the reference's loader does.  ``solver_steps = N`` then assigns
    ``DPMSolverMultistepScheduler(num_train_timesteps=model.noise_steps)`` and ``noise_steps = N`` in the same way: the
    loaded model samples with DPM-Solver++ (2M) in N steps.  ``use_ema=True``: the checkpoint's averaged
    weights (``load_from_checkpoint(use_ema=True)``); it needs a checkpoint file."""
    if model_name not in ("DDPM", "DDIM"):
        raise ValueError("model_name must be 'DDPM' or 'DDIM'")
    cls = Diffusion_DDPM if model_name == "DDPM" else Diffusion_DDIM
    if checkpoint_path is not None and not isinstance(checkpoint_path, (str, bytes)) and not hasattr(checkpoint_path, "__fspath__"):
        state_dict, checkpoint_path = checkpoint_path, None        # load_model(name, state_dict) of earlier callers
    if use_ema:
        if checkpoint_path is None:
            raise ValueError("use_ema=True loads a checkpoint's ema_state_dict: pass a checkpoint file")
        hparams["use_ema"] = True
    if checkpoint_path is not None:
        model = cls.load_from_checkpoint(checkpoint_path, hparams_file=hparams_path, **hparams)
    else:
        model = cls(state_dict=state_dict, **hparams)
    if model_name == "DDIM":
        model.noise_scheduler = DDIMScheduler(num_train_timesteps=num_of_ddim_steps, beta_schedule="linear",
                                              clip_sample=False, prediction_type="epsilon")
        model.noise_steps = num_of_ddim_steps
    if solver_steps is not None:
        model.noise_scheduler = DPMSolverMultistepScheduler(num_train_timesteps=model.noise_steps)
        model.noise_steps = int(solver_steps)
    model.eval()
    return model
