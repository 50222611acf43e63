"""Observation front end: the encoder of the reference's lightweight autoencoder on the GPU.

Mirror of ``self.vision_encoder`` in ``Diffusion_DDPM`` (models/diffusion_ddpm.py:84-88: ``vision.encoder`` of
models/encoder/autoencoder.py:11-20, an ``nn.Sequential`` whose state_dict keys are ``0.weight 0.bias 2.* 4.* 7.*``),
called by ``prepare_obs_cond_vectors`` (:317-321) on ``(B*obs_h, 3, 96, 96)`` frames.  All compute is in
libspdm_hip.so (``spdm_encoder_*``, csrc/encoder.hip + the product's GEMM); there is no CPU path here.

The reference trains this encoder jointly with the U-Net (``Adam(self.parameters())``, :115-116).  ``train_forward`` /
``backward`` / ``update_weights`` are that path (csrc/encoder_train.hip); ``Diffusion_DDPM(...,
train_vision_encoder=True)`` drives them.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .weights import pack_state_dict

ENCODER_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "7.weight", "7.bias")
LATENT_DIM = 128


def feature_columns(observation_dim: int, latent_dim: int = LATENT_DIM) -> slice:
    """The columns of one observed row of ``obs_cond`` that hold the encoder's latents.  ``prepare_obs_cond_vectors``
    concatenates position | action | velocity | features (models/diffusion_ddpm.py:323-330), so they are the last
    ``latent_dim`` of ``observation_dim``."""
    if observation_dim < latent_dim:
        raise ValueError(f"observation_dim {observation_dim} has no room for {latent_dim} image features")
    return slice(observation_dim - latent_dim, observation_dim)


def feature_grad(grad_cond: torch.Tensor, obs_horizon: int, observation_dim: int, latent_dim: int = LATENT_DIM) -> torch.Tensor:
    """d loss / d latents ``(B * obs_horizon, latent_dim)`` out of d loss / d obs_cond (any shape with
    ``obs_horizon * observation_dim`` values per sample): row ``b * obs_horizon + h`` belongs to frame ``h`` of sample
    ``b``, the order of ``img.flatten(end_dim=1)`` (:319)."""
    g = grad_cond.reshape(-1, obs_horizon, observation_dim)
    return g[:, :, feature_columns(observation_dim, latent_dim)].reshape(-1, latent_dim).contiguous()


ENCODER_SHAPES = {"0.weight": (16, 3, 2, 2), "0.bias": (16,), "2.weight": (32, 16, 2, 2), "2.bias": (32,),
                  "4.weight": (64, 32, 2, 2), "4.bias": (64,), "7.weight": (128, 9216), "7.bias": (128,)}


def encoder_state_dict_from(sd, prefix: str = "vision_encoder."):
    """Pick the encoder's tensors out of a diffusion checkpoint's state_dict (keys ``vision_encoder.N.*``) or an
    autoencoder checkpoint's (``encoder.N.*`` / ``model.encoder.N.*``).  Returns None when they are not there."""
    for pre in (prefix, "encoder.", "model.encoder.", ""):
        if all((pre + k) in sd for k in ENCODER_KEYS):
            return {k: sd[pre + k] for k in ENCODER_KEYS}
    return None


class _FrameHandle:
    """What ``VisionEncoder`` and ``autoencoder.Decoder`` share: one ``spdm_<_what>_*`` handle (csrc/spdm_api.hip's
    FrameNet) made from the ``_keys`` / ``_shapes`` tensors of a state_dict, its weights as one flat parameter in the
    packed layout, the flat gradient of the last ``backward`` and the inputs of the pending ``_pass``."""

    _keys, _shapes, _what, _pass = (), {}, "", ""

    def __init__(self, state_dict, device: int = 0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs a visible MI355X (HIP device); there is no CPU fallback")
        self.device = torch.device("cuda", device)
        blob, idx = self._pack(state_dict)
        self._index = [(e.name.decode(), int(e.offset), tuple(e.shape[d] for d in range(e.ndim))) for e in idx]
        self._blob = blob                      # host values at creation; the device copy below follows updates
        self._n_floats = int(blob.size)
        self._flat = None                      # flat_parameter()
        self._grad = None                      # flat gradient of the last backward
        self._pending = None                   # inputs of the pending training forward
        h = ctypes.c_void_p()
        _lib.check(getattr(self.lib, f"spdm_{self._what}_create")(device, blob.ctypes.data_as(ctypes.c_void_p), blob.size, idx,
                                                                 len(idx), ctypes.byref(h)), f"spdm_{self._what}_create")
        self._h = h

    @classmethod
    def _pack(cls, state_dict):
        """The ``_keys`` tensors of ``state_dict``, shapes checked, as ``pack_state_dict``'s (flat fp32 blob, index)."""
        sd = {k: state_dict[k] for k in cls._keys}
        for k, shp in cls._shapes.items():
            if tuple(sd[k].shape) != shp:
                raise ValueError(f"{cls._what} tensor {k}: shape {tuple(sd[k].shape)}, expected {shp}")
        return pack_state_dict(sd)

    def load_state_dict(self, state_dict) -> None:
        """Put a state_dict's values into the handle IN PLACE (``update_weights``): the flat parameter, if it exists, keeps
        its address, so an optimiser configured over it keeps pointing at the weights."""
        self.update_weights(torch.from_numpy(self._pack(state_dict)[0]).to(self.device))

    def close(self):
        if getattr(self, "_h", None):
            getattr(self.lib, f"spdm_{self._what}_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval(self):
        return self

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _run(self, entry: str, *args):
        """``spdm_<_what>_<entry>(handle, *args, stream)`` on the current stream, tensors passed as their device pointers."""
        args = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        name = f"spdm_{self._what}_{entry}"
        _lib.check(getattr(self.lib, name)(self._h, *args, self._stream()), name)

    def _backward_done(self, flat: torch.Tensor) -> None:
        self._pending = None
        self._grad = flat
        if self._flat is not None:
            self._flat.grad = flat

    def grads(self):
        """state_dict name -> gradient of the last ``backward`` (torch layout, views of the flat gradient)."""
        if self._grad is None:
            raise RuntimeError(f"no gradients: call {self._pass} and backward first")
        return {name: self._grad[off:off + int(torch.Size(shape).numel())].view(shape) for name, off, shape in self._index}

    def flat_parameter(self) -> torch.nn.Parameter:
        """The weights as ONE device parameter in the packed layout, created on first use from the values at construction
        (or of the last ``update_weights``); ``backward`` sets its ``.grad``, ``update_weights(p.detach())`` puts an
        optimiser's step into the handle."""
        if self._flat is None:
            self._flat = torch.nn.Parameter(torch.from_numpy(self._blob).to(self.device))
        return self._flat

    def update_weights(self, dev_blob: torch.Tensor, *, follow: bool = True) -> None:
        """Put new values (a device blob in the packed layout, e.g. ``flat_parameter().detach()``) into the handle in
        place; a pending training forward is dropped.  ``follow=False``: the handle alone takes them -- the flat parameter
        and ``state_dict()`` keep their values (a temporary swap: ``Diffusion_DDPM.ema_weights``, which puts them back)."""
        b = dev_blob.detach()
        if b.device != self.device or b.dtype != torch.float32 or not b.is_contiguous() or b.numel() != self._n_floats:
            raise ValueError(f"expected a contiguous fp32 blob of {self._n_floats} floats on {self.device}")
        self._run("update_weights", b, b.numel())
        self._pending = None
        if not follow:
            return
        if self._flat is None:
            self._blob = b.cpu().numpy()
        elif b.data_ptr() != self._flat.data_ptr():      # values from elsewhere: the parameter follows the handle
            with torch.no_grad():
                self._flat.copy_(b)

    def state_dict(self):
        """Current values under the nn.Sequential's key names (host tensors), e.g. for a checkpoint's ``vision_encoder.*``."""
        host = self._flat.detach().cpu().numpy() if self._flat is not None else self._blob
        return {name: torch.from_numpy(host[off:off + int(torch.Size(shape).numel())].reshape(shape).copy())
                for name, off, shape in self._index}


class VisionEncoder(_FrameHandle):
    """``VisionEncoder(state_dict)(images)`` == ``Autoencoder().encoder(images)`` (eval mode), images ``(N,3,96,96)``
    fp32 on the GPU -> ``(N,128)``."""

    _keys, _shapes, _what, _pass = ENCODER_KEYS, ENCODER_SHAPES, "encoder", "train_forward"

    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, 96, 96):
            raise ValueError(f"expected (N,3,96,96) frames, got {tuple(images.shape)}")
        x = images.to(self.device, torch.float32).contiguous()
        out = torch.empty(x.shape[0], 128, device=self.device, dtype=torch.float32)
        if x.shape[0]:
            self._run("forward", x.shape[0], x, out)
        return out

    # ---- joint training ----
    def train_forward(self, images: torch.Tensor) -> torch.Tensor:
        """``__call__``'s latents, bit for bit, with the activations kept for ONE following ``backward``."""
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, 96, 96) or images.shape[0] == 0:
            raise ValueError(f"expected (N,3,96,96) frames with N > 0, got {tuple(images.shape)}")
        x = images.to(self.device, torch.float32).contiguous()
        out = torch.empty(x.shape[0], LATENT_DIM, device=self.device, dtype=torch.float32)
        self._run("train_forward", x.shape[0], x, out)
        self._pending = x
        return out

    def backward(self, grad_latent: torch.Tensor) -> torch.Tensor:
        """d loss / d parameters as ONE flat tensor in the packed layout (``grads()`` are views of it), from
        d loss / d latents ``(N,128)`` of the frames last given to ``train_forward``.  Sets ``flat_parameter().grad``."""
        n = 0 if self._pending is None else self._pending.shape[0]
        g = grad_latent.to(self.device, torch.float32).contiguous()
        if n and tuple(g.shape) != (n, LATENT_DIM):
            raise ValueError(f"grad_latent {tuple(g.shape)}; the pending train_forward had {n} frames")
        if not n:                              # (the library answers SPDM_ERR_STATE; pass valid pointers to reach that answer)
            n, frames = max(int(g.shape[0]), 1), g
        else:
            frames = self._pending
        flat = torch.empty(self._n_floats, device=self.device, dtype=torch.float32)
        self._run("backward", n, frames, g, flat)
        self._backward_done(flat)
        return flat


