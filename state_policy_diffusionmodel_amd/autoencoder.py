"""The reference's lightweight autoencoder on the GPU: the stage that produces the encoder checkpoint
``Diffusion_DDPM`` loads (models/diffusion_ddpm.py:84-88).

Mirror of models/encoder/autoencoder.py: ``Autoencoder`` (:7-37, encoder -> decoder) inside the LightningModule
``autoencoder`` (:40-83, ``MSELoss(recon, batch)``, Adam + ReduceLROnPlateau), which models/encoder/train_autoencoder.py
trains with ``gradient_clip_val=0.5``.  The encoder half is ``vision.VisionEncoder``; ``Decoder`` here is
``Autoencoder.decoder`` (:23-32), an ``nn.Sequential`` whose state_dict keys are ``0.weight 0.bias 2.* 4.* 6.*``.  All
compute is in libspdm_hip.so (``spdm_decoder_*``, csrc/decoder.hip); there is no CPU path here; the
optimiser is torch's or, ``configure_optimizers(device_optimizer=True)``, ``optim.DeviceAdam``.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .vision import ENCODER_KEYS, LATENT_DIM, VisionEncoder, _FrameHandle, encoder_state_dict_from
from .weights import safe_load_state_dict

DECODER_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "6.weight", "6.bias")
DECODER_SHAPES = {"0.weight": (9216, 128), "0.bias": (9216,), "2.weight": (64, 32, 2, 2), "2.bias": (32,),
                  "4.weight": (32, 16, 2, 2), "4.bias": (16,), "6.weight": (16, 3, 2, 2), "6.bias": (3,)}
FRAME = (3, 96, 96)


def decoder_state_dict_from(sd, prefix: str = "decoder."):
    """Pick the decoder's tensors out of an autoencoder checkpoint's state_dict (``decoder.N.*`` /
    ``model.decoder.N.*``) or a bare decoder state_dict.  Returns None when they are not there."""
    for pre in (prefix, "decoder.", "model.decoder.", ""):
        if all((pre + k) in sd for k in DECODER_KEYS):
            return {k: sd[pre + k] for k in DECODER_KEYS}
    return None


def _default_init() -> Dict[str, torch.Tensor]:
    """Both halves with torch's default initialisers for these layers, in checkpoint key names (``encoder.N.*`` /
    ``decoder.N.*``).  Parameter creation only: the modules are never run."""
    nn = torch.nn
    enc = nn.Sequential(nn.Conv2d(3, 16, 2, stride=2, padding=1), nn.ReLU(), nn.Conv2d(16, 32, 2, stride=2), nn.ReLU(),
                        nn.Conv2d(32, 64, 2, stride=2), nn.ReLU(), nn.Flatten(), nn.Linear(64 * 12 * 12, LATENT_DIM))
    dec = nn.Sequential(nn.Linear(LATENT_DIM, 64 * 12 * 12), nn.Unflatten(1, (64, 12, 12)),
                        nn.ConvTranspose2d(64, 32, 2, stride=2), nn.ReLU(), nn.ConvTranspose2d(32, 16, 2, stride=2), nn.ReLU(),
                        nn.ConvTranspose2d(16, 3, 2, stride=2), nn.Sigmoid())
    sd = {"encoder." + k: v.detach().clone() for k, v in enc.state_dict().items()}
    sd.update({"decoder." + k: v.detach().clone() for k, v in dec.state_dict().items()})
    return sd


class Decoder(_FrameHandle):
    """``Decoder(state_dict)(latents)`` == ``Autoencoder().decoder(latents)``, latents ``(N,128)`` fp32 on the GPU ->
    reconstructions ``(N,3,96,96)``."""

    _keys, _shapes, _what, _pass = DECODER_KEYS, DECODER_SHAPES, "decoder", "train_loss"
    recon = None                               # reconstruction of the last train_loss

    def _latents(self, latents: torch.Tensor) -> torch.Tensor:
        if latents.dim() != 2 or latents.shape[1] != LATENT_DIM:
            raise ValueError(f"expected (N,{LATENT_DIM}) latents, got {tuple(latents.shape)}")
        return latents.detach().to(self.device, torch.float32).contiguous()

    def __call__(self, latents: torch.Tensor) -> torch.Tensor:
        z = self._latents(latents)
        out = torch.empty(z.shape[0], *FRAME, device=self.device, dtype=torch.float32)
        if z.shape[0]:
            self._run("forward", z.shape[0], z, out)
        return out

    def train_loss(self, latents: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """``MSELoss(decoder(latents), target)`` as a device scalar, with the activations kept for ONE following
        ``backward``.  ``self.recon`` is the reconstruction, ``__call__``'s bit for bit."""
        z = self._latents(latents)
        if z.shape[0] == 0 or tuple(target.shape) != (z.shape[0], *FRAME):
            raise ValueError(f"expected N > 0 latents and (N,3,96,96) targets, got {tuple(z.shape)} and {tuple(target.shape)}")
        t = target.detach().to(self.device, torch.float32).contiguous()
        recon = torch.empty_like(t)
        loss = torch.empty((), device=self.device, dtype=torch.float32)
        self._run("train_loss", z.shape[0], z, t, recon, loss)
        self._pending = (z, t)
        self.recon = recon
        return loss

    def backward(self):
        """``(flat_grad, grad_latent)`` of the pending ``train_loss``: d loss / d parameters as ONE flat tensor in the
        packed layout (``grads()`` are views of it) and d loss / d latents ``(N,128)``, what ``VisionEncoder.backward``
        takes.  Sets ``flat_parameter().grad``."""
        if self._pending is None:              # (the library answers SPDM_ERR_STATE; pass valid pointers to reach that answer)
            z = torch.zeros(1, LATENT_DIM, device=self.device)
            t = torch.zeros(1, *FRAME, device=self.device)
        else:
            z, t = self._pending
        flat = torch.empty(self._n_floats, device=self.device, dtype=torch.float32)
        gl = torch.empty(z.shape[0], LATENT_DIM, device=self.device, dtype=torch.float32)
        self._run("backward", z.shape[0], z, t, flat, gl)
        self._backward_done(flat)
        return flat, gl


class autoencoder:
    """The reference's LightningModule surface (models/encoder/autoencoder.py:40-83) over the two HIP handles.

    ``state_dict``: an autoencoder checkpoint's (``encoder.N.*`` / ``model.encoder.N.*`` and the decoder's likewise) or
    None for torch's default initialisation of these layers."""

    def __init__(self, learning_rate: float = 1e-3, state_dict=None, device: int = 0):
        self.lr = learning_rate
        sd = _default_init() if state_dict is None else state_dict
        enc_sd, dec_sd = encoder_state_dict_from(sd, "encoder."), decoder_state_dict_from(sd)
        if enc_sd is None or dec_sd is None:
            raise ValueError("state_dict holds no autoencoder: expected encoder.N.* (0, 2, 4, 7) and decoder.N.* (0, 2, 4, 6)")
        self.encoder = VisionEncoder(enc_sd, device=device)
        self.decoder = Decoder(dec_sd, device=device)
        self.device = self.decoder.device

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, learning_rate: float = 1e-3, device: int = 0):
        """From a Lightning ``.ckpt`` of the reference's ``autoencoder`` (or a bare state_dict file), read with
        ``torch.load(weights_only=True)`` only."""
        return cls(learning_rate, safe_load_state_dict(str(checkpoint_path)), device)

    def close(self):
        self.encoder.close()
        self.decoder.close()

    def eval(self):
        return self

    # ==================== Forward (Autoencoder.forward, :34-37) ====================
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.decoder(self.encoder(x))

    __call__ = forward

    # ==================== Training (:55-71) ====================
    def training_step(self, batch: torch.Tensor, batch_idx: int = 0, *, backward: bool = False) -> torch.Tensor:
        """``MSELoss(decoder(encoder(batch)), batch)`` as a device scalar.  ``backward=True`` also backpropagates: the
        gradients are then in ``encoder.grads()`` / ``decoder.grads()`` and on both flat parameters' ``.grad``."""
        x = batch.detach().to(self.device, torch.float32).contiguous()
        if not backward:
            return self.decoder.train_loss(self.encoder(x), x)
        self._params()                          # (the flat parameters exist before the backward passes: both get their .grad)
        loss = self.decoder.train_loss(self.encoder.train_forward(x), x)
        _, grad_latent = self.decoder.backward()
        self.encoder.backward(grad_latent)
        return loss

    def validation_step(self, batch: torch.Tensor, batch_idx: int = 0) -> torch.Tensor:
        return self.training_step(batch, batch_idx)

    # ==================== Optimisation (:73-83, train_autoencoder.py) ====================
    def _params(self):
        return [self.encoder.flat_parameter(), self.decoder.flat_parameter()]

    def configure_optimizers(self, device_optimizer: bool = False):
        """Adam(lr) over the two flat device parameters -- Adam is elementwise, so this is ``Adam(self.parameters())`` --
        and ReduceLROnPlateau('min', patience=5) on ``val_loss``, in Lightning's dict shape.  ``device_optimizer=True``:
        the same dict with ``optim.DeviceAdam`` (clip + Adam in HIP) in torch.optim.Adam's place."""
        if device_optimizer:
            from .optim import DeviceAdam
            optimizer = DeviceAdam(self._params(), lr=self.lr)
        else:
            optimizer = torch.optim.Adam(self._params(), lr=self.lr)
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
        """One optimiser step after ``training_step(backward=True)``: clip the global gradient norm over both halves
        (Lightning's ``gradient_clip_val``, 0.5 in train_autoencoder.py), ``optimizer.step()``, then put the new weights
        into both handles in place."""
        params = self._params()
        from .optim import DeviceAdam
        if isinstance(optimizer, DeviceAdam):       # clip over both halves + Adam in two HIP launches
            optimizer.step(max_norm=gradient_clip_val or None)
            self.encoder.update_weights(params[0].detach())
            self.decoder.update_weights(params[1].detach())
            return
        if gradient_clip_val:
            torch.nn.utils.clip_grad_norm_(params, gradient_clip_val)
        optimizer.step()
        self.encoder.update_weights(params[0].detach())
        self.decoder.update_weights(params[1].detach())

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The Lightning checkpoint's keys: ``model.encoder.N.*`` / ``model.decoder.N.*`` and the aliases
        ``encoder.N.*`` / ``decoder.N.*`` (:49-51 registers the same modules twice).  ``Diffusion_DDPM(...,
        vision_encoder_state_dict=...)`` accepts it as it is."""
        out = {}
        for pre in ("model.", ""):
            out.update({f"{pre}encoder.{k}": v for k, v in self.encoder.state_dict().items()})
            out.update({f"{pre}decoder.{k}": v for k, v in self.decoder.state_dict().items()})
        return out


__all__ = ["DECODER_KEYS", "DECODER_SHAPES", "ENCODER_KEYS", "Decoder", "autoencoder", "decoder_state_dict_from"]
