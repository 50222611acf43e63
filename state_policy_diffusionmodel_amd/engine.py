"""SpdmEngine -- thin Python owner of one ``spdm_handle`` (include/spdm.h).

PyTorch-ROCm tensors are used for interop only (device memory, streams): every
call hands ``data_ptr()`` / the current HIP stream to the C ABI; all compute is
in libspdm_hip.so.  No CPU path exists here.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from .weights import is_simple_model, pack_state_dict, unet_film_param_spec, unet_simple_param_spec


def reference_time_table(T: int, channels: int = 256) -> torch.Tensor:
    """pos_encoding(t) for t = 0..T-1 with torch's own fp32 ops in the reference's order
    (models/Unet_FiLmLayer.py:266-274 applied to ``t.unsqueeze(-1).float()``, :281)."""
    t = torch.arange(T, dtype=torch.int64).unsqueeze(-1).type(torch.float)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, channels, 2) / channels))
    a = torch.sin(t.repeat(1, channels // 2) * inv_freq)
    b = torch.cos(t.repeat(1, channels // 2) * inv_freq)
    return torch.cat([a, b], dim=-1).contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def solver_step(eps: torch.Tensor, x: torch.Tensor, x0_prev: torch.Tensor, coef: torch.Tensor, step: int, first: int,
                words: torch.Tensor, inpaint: Optional[torch.Tensor] = None, history: Optional[torch.Tensor] = None) -> None:
    """One DPM-Solver++ (2M) update in place on the caller's device tensors (``spdm_solver_step``, include/spdm.h): the launch
    the library's own loop makes, for callers that drive the loop themselves.  ``eps``, ``x``, ``x0_prev`` (B,H,D) or
    (B,1,H,D) float32; ``coef`` (n,6) float32, a scheduler's ``coefficient_table()`` on the device; ``words`` int32[3]
    ({step, first, non-finite flag}: the flag is only ever set); ``inpaint`` (inp_h,D) or (B,inp_h,D); ``history``
    (n+1,B,H,D), row ``step + 1`` receives the new iterate.  ``first``: the iteration that has no history term, or -1."""
    B, H, D = x.shape[0], x.shape[-2], x.shape[-1]
    given = [("eps", eps), ("x", x), ("x0_prev", x0_prev), ("coef", coef)] + ([("inpaint", inpaint)] if inpaint is not None else [])
    given += [("history", history)] if history is not None else []
    for name, t in given:
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"{name} must be a contiguous float32 tensor on {x.device}")
    if eps.numel() != x.numel() or x0_prev.numel() != x.numel() or x.numel() != B * H * D:
        raise ValueError("eps, x and x0_prev must all be (B,H,D) or (B,1,H,D)")
    if coef.dim() != 2 or coef.shape[1] != 6:
        raise ValueError(f"coef must be (n,6), got {tuple(coef.shape)}")
    if not words.is_cuda or words.dtype != torch.int32 or words.numel() < 3 or not words.is_contiguous() or words.device != x.device:
        raise ValueError("words must be a contiguous int32 device tensor of 3 elements")
    n, inp_h, per_sample = int(coef.shape[0]), 0, 0
    if inpaint is not None:
        inp_h = int(inpaint.shape[-2])
        per_sample = int(inpaint.numel() == B * inp_h * D and B > 1)
        if inpaint.shape[-1] != D or inpaint.numel() not in (inp_h * D, B * inp_h * D):
            raise ValueError(f"inpaint must be (inp_h,{D}) or ({B},inp_h,{D}), got {tuple(inpaint.shape)}")
    if history is not None and history.numel() != (n + 1) * B * H * D:
        raise ValueError(f"history must be ({n + 1},{B},{H},{D})")
    a = _lib.SpdmSolverStepArgs(B=B, H=H, D=D, inp_h=inp_h, inpaint_per_sample=per_sample, n_steps=n, step=int(step),
                                first=int(first), d_eps=eps.data_ptr(), d_x=x.data_ptr(), d_x0_prev=x0_prev.data_ptr(),
                                d_coef=coef.data_ptr(), d_inpaint=inpaint.data_ptr() if inp_h > 0 else None,
                                d_history=history.data_ptr() if history is not None else None, d_words=words.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(_lib.load().spdm_solver_step(x.device.index, ctypes.byref(a), stream), "spdm_solver_step")


class SpdmEngine:
    def __init__(self, horizon: int, state_dim: int, cond_dim: int, max_batch: int, device: int = 0,
                 attention: bool = True, time_dim: int = 256, num_train_timesteps: int = 1000,
                 debug: bool = False, exact_fp32: bool = False, pin_geometry: bool = False,
                 model: Optional[str] = None, train: bool = False, train_attention: bool = False,
                 train_simple: bool = False):
        """``model``: None -> UNet_Film (``attention=True``) / UNet_FilmnoAttention (``attention=False``); a model name as
        Diffusion_DDPM takes it otherwise -- ``'UNet'`` (any non-FiLM name) is models/simple_Unet.py's network, whose
        time table is the state_dict's own ``pos_encoding.pos_encoding`` buffer: ``num_train_timesteps`` must then be
        that buffer's row count (noise_steps + 1).

        ``train``: the handle also serves ``loss_and_grad`` (SPDM_FLAG_TRAIN; UNet_FilmnoAttention only).
        ``train_attention``: ``loss_and_grad`` for UNet_Film, through its SelfAttention blocks (SPDM_FLAG_TRAIN |
        SPDM_FLAG_TRAIN_ATTENTION); needs the FiLM model with attention and implies ``train``.
        ``train_simple``: ``loss_and_grad`` for simple_Unet.py's UNet (SPDM_FLAG_TRAIN | SPDM_FLAG_TRAIN_SIMPLE); needs
        ``model='UNet'`` and implies ``train``."""
        self.lib = _lib.load()
        self.simple = model is not None and is_simple_model(model)
        if model is not None and not self.simple:
            attention = model == "UNet_Film"
        if self.simple:
            attention = False
        if train_attention:
            if self.simple or not attention:
                raise ValueError("train_attention=True needs UNet_Film (the FiLM model with attention)")
            train = True
        if train_simple:
            if not self.simple:
                raise ValueError("train_simple=True needs model='UNet' (simple_Unet.py's network)")
            train = True
        if not torch.cuda.is_available():
            raise RuntimeError("SpdmEngine needs a visible MI355X (HIP device); there is no CPU fallback")
        self.device = torch.device("cuda", device)
        self.horizon, self.state_dim, self.cond_dim = int(horizon), int(state_dim), int(cond_dim)
        self.max_batch, self.attention, self.time_dim = int(max_batch), bool(attention), int(time_dim)
        self.num_train_timesteps = int(num_train_timesteps)
        cfg = _lib.SpdmConfig(self.horizon, self.state_dim, self.cond_dim, self.time_dim, int(self.attention),
                              self.max_batch, device, self.num_train_timesteps,
                              (_lib.SPDM_FLAG_DEBUG_KEEP if debug else 0) | (_lib.SPDM_FLAG_EXACT_FP32 if exact_fp32 else 0)
                              | (_lib.SPDM_FLAG_SIMPLE_UNET if self.simple else 0) | (_lib.SPDM_FLAG_TRAIN if train else 0)
                              | (_lib.SPDM_FLAG_TRAIN_ATTENTION if train_attention else 0)
                              | (_lib.SPDM_FLAG_TRAIN_SIMPLE if train_simple else 0))
        self.train = bool(train)
        self.train_attention = bool(train_attention)
        self.train_simple = bool(train_simple)
        self._cfg = cfg
        self._pin = bool(pin_geometry)
        self._create()
        self._keep = []           # tensors the C side reads asynchronously during a session
        self.n_steps = 0
        self.kind = None
        self._weights_loaded = False
        self._sched = None
        self._switches = {}
        self._rebuilds = 0

    def _create(self) -> None:
        h = ctypes.c_void_p()
        _lib.check(self.lib.spdm_create(ctypes.byref(self._cfg), ctypes.byref(h)), "spdm_create")
        self._h = h
        if self._pin:
            # kernel selection (tile sizes, split-K, the small-grid kernel, fused sources) normally follows the batch of the call;
            # pinned, every call runs the kernels a batch of max_batch would -- so a rank that holds a shard of a larger batch
            # (max_batch = the GLOBAL batch) reproduces the single-GPU trajectories bit for bit (multi-GPU)
            _lib.check(self.lib.spdm_set_switch(self._h, b"SPDM_PIN_GEOMETRY", 1), "spdm_set_switch")
        if not self.simple:        # (simple_Unet.py: the table is the state_dict's pos_encoding buffer, set by load_state_dict)
            tab = reference_time_table(self.num_train_timesteps, self.time_dim).numpy()
            _lib.check(self.lib.spdm_set_time_table(self._h, tab.ctypes.data_as(ctypes.c_void_p),
                                                    self.num_train_timesteps), "spdm_set_time_table")

    # -- lifetime -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.spdm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def split_precision(self) -> bool:
        """True: contractions on the split-fp16 MFMA path (default); False: exact fp32 MFMA."""
        return bool(self.lib.spdm_uses_split_precision(self._h))

    @property
    def device_bytes(self) -> int:
        return int(self.lib.spdm_device_bytes(self._h))

    @property
    def demoted_tensors(self) -> int:
        """Weight tensors outside the split format's range (|w| >= 511), kept on the exact fp32 kernels."""
        return int(self.lib.spdm_demoted_tensors(self._h))

    @property
    def graph_captures(self) -> int:
        """Step graphs captured so far: stays at 1 across sample() calls of one shape, whatever tensors they pass."""
        return int(self.lib.spdm_graph_captures(self._h))

    def set_switch(self, name: str, on: bool = True) -> None:
        """Flip one kernel-selection switch (``SPDM_NO_GRAPH``, ``SPDM_NO_WIDE``, ...) on this handle.  The
        environment is read once, at construction; this is the test / tuning hook for a live engine."""
        _lib.check(self.lib.spdm_set_switch(self._h, name.encode(), int(bool(on))), "spdm_set_switch")
        self._switches[name] = bool(on)

    def nonfinite(self) -> bool:
        """True if the last sampling loop / U-Net evaluation produced a non-finite value (synchronises the stream).
        On the split-precision path this is how an activation beyond its range (|x| > 4094) shows."""
        flag = ctypes.c_int32(0)
        _lib.check(self.lib.spdm_nonfinite(self._h, ctypes.byref(flag), self._stream()), "spdm_nonfinite")
        return bool(flag.value)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t: Optional[torch.Tensor], shape=None, name="tensor") -> Optional[torch.Tensor]:
        if t is None:
            return None
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            t = t.reshape(shape)
        return t

    # -- setup --------------------------------------------------------------------------------
    def load_state_dict(self, sd) -> None:
        """state_dict of the reference noise predictor (names as ``UNet_Film.state_dict()``;
        a Lightning checkpoint's ``noise_estimator.`` prefix is stripped)."""
        blob, idx = pack_state_dict(sd)
        if self.simple:
            want = set(unet_simple_param_spec(self.cond_dim, self.num_train_timesteps - 1, self.time_dim).keys())
        else:
            want = set(unet_film_param_spec(self.cond_dim, self.time_dim, self.attention).keys())
        have = {e.name.decode() for e in idx}
        missing = sorted(want - have)
        if missing:
            raise KeyError(f"state_dict lacks {len(missing)} tensors, e.g. {missing[:3]}")
        if self._weights_loaded and self.train:
            self.refresh_weights(sd)
            return
        _lib.check(self.lib.spdm_load_weights(self._h, blob.ctypes.data_as(ctypes.c_void_p), blob.size, idx,
                                              len(idx)), "spdm_load_weights")
        self._weights_loaded = True
        self._index = [(e.name.decode(), int(e.offset), tuple(e.shape[d] for d in range(e.ndim))) for e in idx]
        self._blob_floats = int(blob.size)

    def refresh_weights(self, sd) -> None:
        """Put updated weights (an optimiser step) into this engine.  A handle takes its weights once, so a fresh handle of the
        same configuration is created, loaded (spdm_load_weights), given the installed schedule and switches, and only then
        replaces the old one: on any failure the engine keeps its previous handle and weights.  Costs a handle creation per
        call (tools/bench_train.py times it as the host weight refresh)."""
        old, old_keep = self._h, self._keep
        self._create()
        try:
            blob, idx = pack_state_dict(sd)
            _lib.check(self.lib.spdm_load_weights(self._h, blob.ctypes.data_as(ctypes.c_void_p), blob.size, idx,
                                                  len(idx)), "spdm_load_weights")
            for name, on in self._switches.items():
                _lib.check(self.lib.spdm_set_switch(self._h, name.encode(), int(on)), "spdm_set_switch")
            if self._sched is not None:
                self._sched()
        except Exception:
            self.lib.spdm_destroy(self._h)
            self._h, self._keep = old, old_keep
            raise
        self.lib.spdm_destroy(old)
        self._keep = []
        self._weights_loaded = True
        self._index = [(e.name.decode(), int(e.offset), tuple(e.shape[d] for d in range(e.ndim))) for e in idx]
        self._blob_floats = int(blob.size)

    def pack_weights(self, sd) -> torch.Tensor:
        """state_dict -> one flat fp32 tensor on the engine's device laid out as the loaded blob (the layout of
        ``update_weights`` and ``loss_and_grad(flat=True)``).  Raises ValueError if the names, shapes or offsets differ
        from the loaded index."""
        if not self._weights_loaded:
            raise RuntimeError("load_state_dict first")
        blob, idx = pack_state_dict(sd)
        index = [(e.name.decode(), int(e.offset), tuple(e.shape[d] for d in range(e.ndim))) for e in idx]
        if index != self._index or int(blob.size) != self._blob_floats:
            raise ValueError("state_dict does not pack into the loaded blob's layout (names, shapes or offsets differ)")
        return torch.from_numpy(blob).to(self.device)

    def unpack_weights(self, flat: torch.Tensor) -> dict:
        """The inverse of ``pack_weights``: name -> host numpy array (a copy)."""
        host = flat.detach().to("cpu", torch.float32).numpy()
        out = {}
        for name, off, shape in self._index:
            n = int(np.prod(shape)) if shape else 1
            out[name] = host[off:off + n].reshape(shape).copy()
        return out

    def update_weights(self, flat: torch.Tensor) -> None:
        """Put updated weights (an optimiser step) into this engine in place: ``flat`` is a contiguous fp32 tensor on the
        engine's device in the packed layout (``pack_weights``).  The re-layout runs on the current stream; ``flat`` must
        stay unchanged until that stream has passed it.  If the set of tensors outside the split format's range
        (``demoted_tensors``) would change, the handle is rebuilt from a host copy instead (``refresh_weights``;
        counted by ``weight_rebuilds``)."""
        if not self._weights_loaded:
            raise RuntimeError("load_state_dict first")
        if (flat.device != self.device or flat.dtype != torch.float32 or not flat.is_contiguous()
                or flat.numel() != self._blob_floats):
            raise ValueError(f"update_weights needs a contiguous fp32 tensor of {self._blob_floats} floats on {self.device}")
        rc = self.lib.spdm_update_weights(self._h, _ptr(flat), flat.numel(), self._stream())
        if rc == _lib.SPDM_ERR_STATE:          # the range set changed: the workspace plan depends on it
            self.refresh_weights(self.unpack_weights(flat))
            self._rebuilds += 1
            return
        _lib.check(rc, "spdm_update_weights")

    @property
    def weight_rebuilds(self) -> int:
        """``update_weights`` calls that had to rebuild the handle (a tensor entered or left the split format's range)."""
        return self._rebuilds

    def weight_digest(self) -> int:
        """Hash of every device weight copy, outc's bias and the demotion set (test hook; synchronises the device)."""
        d = ctypes.c_uint64(0)
        _lib.check(self.lib.spdm_debug_weight_digest(self._h, ctypes.byref(d)), "spdm_debug_weight_digest")
        return int(d.value)

    def plan_routes(self, B: int) -> dict:
        """The kernel routes the plan chooses for one U-Net evaluation at batch ``B`` (spdm_debug_plan_routes; test hook, host
        arithmetic only): ``pool`` / ``up`` / ``film``: tuples of 3 / 3 / 6 route codes, ``sa``: six dicts
        {fused, crop, outc, in, tail}, ``chain``: (down block 3, bottleneck) -- the codes are listed in include/spdm.h."""
        v = (ctypes.c_int32 * 44)()
        _lib.check(self.lib.spdm_debug_plan_routes(self._h, int(B), v, len(v)), "spdm_debug_plan_routes")
        v = [int(x) for x in v]
        sa = [dict(zip(("fused", "crop", "outc", "in", "tail"), v[12 + 5 * i:17 + 5 * i])) for i in range(6)]
        return {"pool": tuple(v[0:3]), "up": tuple(v[3:6]), "film": tuple(v[6:12]), "sa": sa, "chain": tuple(v[42:44])}

    def set_scheduler(self, sched) -> None:
        """Install the tables of a host scheduler object (schedulers.py) for the loop."""
        ts = np.ascontiguousarray(np.asarray(sched.timesteps, dtype=np.int64).astype(np.int32))
        coef = np.ascontiguousarray(sched.coefficient_table(), dtype=np.float32)
        assert coef.shape == (ts.size, 6)
        _lib.check(self.lib.spdm_set_schedule_tables(self._h, int(sched.kind), int(ts.size),
                                                     ts.ctypes.data_as(ctypes.c_void_p),
                                                     coef.ctypes.data_as(ctypes.c_void_p)), "spdm_set_schedule_tables")
        self.n_steps, self.kind = int(ts.size), int(sched.kind)
        self._sched = lambda: self.set_scheduler(sched)

    def set_builtin_schedule(self, kind: int, num_train_timesteps: int, num_inference_steps: int,
                             beta_start: float = 1e-4, beta_end: float = 0.02) -> None:
        _lib.check(self.lib.spdm_set_schedule(self._h, kind, num_train_timesteps, num_inference_steps,
                                              beta_start, beta_end), "spdm_set_schedule")
        self.n_steps, self.kind = int(num_inference_steps), int(kind)
        self._sched = lambda: self.set_builtin_schedule(kind, num_train_timesteps, num_inference_steps, beta_start, beta_end)

    # -- the noise predictor ------------------------------------------------------------------
    def unet_forward(self, x: torch.Tensor, t, cond: Optional[torch.Tensor]) -> torch.Tensor:
        """eps = noise_estimator(x, t, cond); x (B,1,H,D), t (1,)|(B,) ints, cond (B,1,obs_h,obs_dim).
        ``t`` as a device int32 tensor of B or 1 elements (``noising.forward_process`` returns one) stays on the device
        (``spdm_unet_forward_dt``): no host copy, values outside [0, T) are clamped into range instead of rejected."""
        B = x.shape[0]
        xs = self._dev(x, (B, self.horizon, self.state_dim))
        cs = self._dev(cond, (B, self.cond_dim)) if cond is not None else None
        eps = torch.empty((B, 1, self.horizon, self.state_dim), device=self.device, dtype=torch.float32)
        if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.numel() in (1, B):
            td = t.to(self.device).reshape(-1).contiguous()
            _lib.check(self.lib.spdm_unet_forward_dt(self._h, B, _ptr(xs), _ptr(td), int(td.numel()), _ptr(cs), _ptr(eps),
                                                     self._stream()), "spdm_unet_forward_dt")
            return eps
        tt = np.ascontiguousarray(torch.as_tensor(t).reshape(-1).cpu().numpy().astype(np.int32))
        _lib.check(self.lib.spdm_unet_forward(self._h, B, _ptr(xs), tt.ctypes.data_as(ctypes.c_void_p), int(tt.size),
                                              _ptr(cs), _ptr(eps), self._stream()), "spdm_unet_forward")
        return eps

    # -- training ---------------------------------------------------------------------------------
    def loss_and_grad(self, x_noisy: torch.Tensor, t, cond: Optional[torch.Tensor], noise: torch.Tensor,
                      flat: bool = False, time_scale: Optional[torch.Tensor] = None):
        """One training step's forward and backward pass (models/diffusion_ddpm.py:128-173): eps = unet(x_noisy, t, cond),
        loss = mean((noise - eps)^2), and the gradients of loss.  Returns ``(loss, eps, grads, grad_cond)``: ``grads`` maps
        every state_dict name to its gradient (torch layout, on the device) -- or, ``flat=True``, is one flat tensor laid
        out as the packed state_dict; ``grad_cond`` is d loss / d cond (None without cond).  For simple_Unet.py's UNet
        (``train_simple=True``) ``grads`` covers its parameters only (not the ``pos_encoding.pos_encoding`` buffer, whose
        slot of the flat tensor holds zeros), and ``time_scale`` (B, time_dim) -- PositionalEncoding's dropout mask over
        (1 - p), e.g. ``F.dropout(torch.ones(B, 256, device='cuda'), 0.1, True)`` -- multiplies pe[t_b] (training mode).
        ``t`` as a device int32 tensor of B or 1 elements (``noising.forward_process`` returns one) stays on the device
        (``spdm_train_loss_grad_dt``): no host copy, values outside [0, T) are clamped into range instead of rejected."""
        if not self.train:
            raise RuntimeError("loss_and_grad needs an engine created with train=True")
        if time_scale is not None and not self.train_simple:
            raise ValueError("time_scale needs an engine created with train_simple=True (simple_Unet.py's UNet)")
        if not self._weights_loaded:
            raise RuntimeError("load_state_dict first")
        B = x_noisy.shape[0]
        H, D = self.horizon, self.state_dim
        xs = self._dev(x_noisy, (B, H, D))
        ns = self._dev(noise, (B, H, D))
        cs = self._dev(cond, (B, self.cond_dim)) if cond is not None else None
        # a device int32 t of B or 1 elements stays where it is (spdm_train_loss_grad_dt: no .cpu() of t and no host range check; the pass's own waits remain)
        td = None
        if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.numel() in (1, B):
            td = t.to(self.device).reshape(-1).contiguous()
        else:
            tt = np.ascontiguousarray(torch.as_tensor(t).reshape(-1).cpu().numpy().astype(np.int32))
        loss = torch.empty((), device=self.device, dtype=torch.float32)
        eps = torch.empty((B, 1, H, D), device=self.device, dtype=torch.float32)
        g = torch.empty(self._blob_floats, device=self.device, dtype=torch.float32)
        gc = torch.empty((B,) + tuple(cond.shape[1:]), device=self.device, dtype=torch.float32) if cs is not None else None
        if time_scale is not None:
            if tuple(time_scale.shape) != (B, self.time_dim):
                raise ValueError(f"time_scale must be (B, time_dim) = ({B}, {self.time_dim}), got {tuple(time_scale.shape)}")
            ts = self._dev(time_scale)
            _lib.check(self.lib.spdm_train_set_time_scale(self._h, _ptr(ts), B), "spdm_train_set_time_scale")
        if td is not None:
            _lib.check(self.lib.spdm_train_loss_grad_dt(self._h, B, _ptr(xs), _ptr(td), int(td.numel()), _ptr(cs), _ptr(ns),
                                                        _ptr(loss), _ptr(eps), _ptr(g), _ptr(gc), self._stream()),
                       "spdm_train_loss_grad_dt")
        else:
            _lib.check(self.lib.spdm_train_loss_grad(self._h, B, _ptr(xs), tt.ctypes.data_as(ctypes.c_void_p), int(tt.size),
                                                     _ptr(cs), _ptr(ns), _ptr(loss), _ptr(eps), _ptr(g), _ptr(gc),
                                                     self._stream()), "spdm_train_loss_grad")
        if flat:
            return loss, eps, g, gc
        grads = {}
        for name, off, shape in self._index:
            if self.simple and name == "pos_encoding.pos_encoding":      # a buffer, not a parameter
                continue
            n = int(np.prod(shape)) if shape else 1
            grads[name] = g[off:off + n].view(shape)
        return loss, eps, grads, gc

    # -- the sampling loop --------------------------------------------------------------------
    def sample_begin(self, cond, x_T, noise=None, inpaint=None, seed: int = 0, sample_offset: int = 0,
                     history: bool = False) -> Optional[torch.Tensor]:
        if self.n_steps <= 0:
            raise RuntimeError("no scheduler installed (set_scheduler)")
        B = x_T.shape[0]
        H, D = self.horizon, self.state_dim
        xs = self._dev(x_T, (B, H, D))
        cs = self._dev(cond, (B, self.cond_dim)) if cond is not None else None
        ns = self._dev(noise, (self.n_steps, B, H, D)) if noise is not None else None
        inp_h, per_sample, ip = 0, 0, None
        if inpaint is not None:
            ip = self._dev(inpaint)
            ip = ip.reshape(-1, ip.shape[-2], ip.shape[-1])
            inp_h = ip.shape[1]
            if ip.shape[2] != D or ip.shape[0] not in (1, B):
                raise ValueError(f"inpaint must be (1|B,1,inp_h,{D}), got {tuple(inpaint.shape)}")
            per_sample = int(ip.shape[0] == B and B > 1)
        hist = torch.empty((self.n_steps + 1, B, 1, H, D), device=self.device, dtype=torch.float32) if history else None
        self._keep = [xs, cs, ns, ip, hist]
        self._B = B
        _lib.check(self.lib.spdm_sample_begin(self._h, B, _ptr(cs), _ptr(ip), inp_h, per_sample, _ptr(xs), _ptr(ns),
                                              ctypes.c_uint64(seed), ctypes.c_uint64(sample_offset), _ptr(hist),
                                              self._stream()), "spdm_sample_begin")
        return hist

    def sample_run(self, step_begin: int, step_end: int) -> None:
        _lib.check(self.lib.spdm_sample_run(self._h, step_begin, step_end, self._stream()), "spdm_sample_run")

    def sample_result(self) -> torch.Tensor:
        out = torch.empty((self._B, 1, self.horizon, self.state_dim), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.spdm_sample_result(self._h, _ptr(out), self._stream()), "spdm_sample_result")
        return out

    def sample(self, cond, x_T, noise=None, inpaint=None, seed: int = 0, sample_offset: int = 0,
               history: bool = False, check_finite: bool = True, start_step: int = 0):
        """x_0 (B,1,H,D); with history=True also the (n_steps+1,B,1,H,D) stack x_T..x_0.  Raises if an iterate left
        the finite range (the split-precision contractions overflow beyond |activation| 4094: re-create the engine
        with exact_fp32=True for such a model).  ``start_step = i0``: ``x_T`` is the iterate after ``i0`` steps and only
        steps ``[i0, n_steps)`` run; there is no history of such a run."""
        if not 0 <= start_step <= self.n_steps:
            raise ValueError(f"start_step = {start_step} outside [0, {self.n_steps}]")
        if start_step and history:
            raise ValueError("history=True needs the whole loop (start_step = 0)")
        hist = self.sample_begin(cond, x_T, noise, inpaint, seed, sample_offset, history)
        self.sample_run(start_step, self.n_steps)
        out = self.sample_result()
        if check_finite and self.nonfinite():
            raise FloatingPointError("non-finite iterate in the sampling loop" + (
                ": an activation left the split-fp16 range (|x| < 4094); use exact_fp32=True" if self.split_precision else ""))
        return (out, hist) if history else out

    def sample_stream(self, cond, x_T, noise=None, inpaint=None, seed: int = 0, sample_offset: int = 0, every: int = 1):
        """Generator over the running loop: yields ``(i, x_i)`` -- the iterate after ``i`` denoise steps as a HOST tensor
        (B,1,H,D) -- for i = 0, every, 2*every, ..., n_steps, WHILE the device keeps stepping: chunk k+1 is enqueued before
        chunk k's snapshot is handed out, and snapshots travel on a side stream into pinned memory.  This is the streaming
        form of ``option='sample_history'`` (models/diffusion_ddpm.py:256-265 builds the whole list first; its consumer,
        utils/plot_utils.py:199-277, draws one frame per iterate)."""
        if every < 1:
            raise ValueError("every must be >= 1")
        self.sample_begin(cond, x_T, noise, inpaint, seed, sample_offset, history=False)
        main = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(device=self.device)
        pending = None                                     # (step index, pinned host tensor, copy-done event)

        def snapshot(i):
            dev_copy = self.sample_result()                # device-side copy, ordered behind step i on the loop's stream
            ready = torch.cuda.Event()
            ready.record(main)
            host = torch.empty(dev_copy.shape, dtype=dev_copy.dtype, pin_memory=True)
            with torch.cuda.stream(side):
                side.wait_event(ready)
                host.copy_(dev_copy, non_blocking=True)
                dev_copy.record_stream(side)
                done = torch.cuda.Event()
                done.record(side)
            return i, host, done

        pending = snapshot(0)
        i = 0
        while i < self.n_steps:
            j = min(self.n_steps, i + every)
            self.sample_run(i, j)                          # asynchronous: the device works on [i, j) ...
            nxt = snapshot(j)
            pi, ph, pd = pending                           # ... while the caller consumes iterate i
            pd.synchronize()
            yield pi, ph
            pending, i = nxt, j
        pi, ph, pd = pending
        pd.synchronize()
        yield pi, ph

    # -- introspection ------------------------------------------------------------------------
    def debug_tensor(self, name: str) -> torch.Tensor:
        """Named intermediate of the last unet_forward as NCHW (engine created with debug=True)."""
        shape = (ctypes.c_int32 * 4)()
        _lib.check(self.lib.spdm_debug_tensor(self._h, name.encode(), ctypes.c_void_p(0), 0, ctypes.byref(shape)),
                   "spdm_debug_tensor")
        B, H, W, C = (int(v) for v in shape)
        buf = torch.empty((B, H, W, C), device=self.device, dtype=torch.float32)
        _lib.check(self.lib.spdm_debug_tensor(self._h, name.encode(), _ptr(buf), buf.numel(), ctypes.byref(shape)),
                   "spdm_debug_tensor")
        return buf.permute(0, 3, 1, 2).contiguous()

    def profile(self, on) -> None:
        """True / False: per-launch HIP events on / off; "prepare": create the events now, instrument nothing yet."""
        mode = 2 if on == "prepare" else int(bool(on))
        _lib.check(self.lib.spdm_profile_enable(self._h, mode), "spdm_profile_enable")

    def profile_read(self):
        n, ms, fl = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _lib.check(self.lib.spdm_profile_read(self._h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)),
                   "spdm_profile_read")
        return int(n.value), float(ms.value), float(fl.value)
