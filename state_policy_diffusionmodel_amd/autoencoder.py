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

import numpy as np
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
    None for torch's default initialisation of these layers -- from the global RNG, or with ``weight_seed`` from a forked
    generator seeded with it, so that two constructions with one seed are bit-equal.  ``train.fit`` drives it
    (train_autoencoder.py)."""

    model_name = "autoencoder"                  # what ``train.fit`` asks a model for (no time dropout, no EMA)

    def __init__(self, learning_rate: float = 1e-3, state_dict=None, device: int = 0, weight_seed: Optional[int] = None):
        self.lr = learning_rate
        if state_dict is not None:
            sd = state_dict
        elif weight_seed is None:
            sd = _default_init()
        else:                                   # a forked, seeded generator: the global RNG stream is left as it was
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(int(weight_seed))
                sd = _default_init()
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
    def training_step(self, batch: torch.Tensor, batch_idx: int = 0, *, backward: bool = False, device_noise=None, seed=None,
                      noise_step=None, time_dropout=None) -> torch.Tensor:
        """``MSELoss(decoder(encoder(batch)), batch)`` as a device scalar.  ``backward=True`` also backpropagates: the
        gradients are then in ``encoder.grads()`` / ``decoder.grads()`` and on both flat parameters' ``.grad``.
        ``device_noise``, ``seed`` and ``noise_step`` are ``train.fit``'s keywords for a step's random draws, and
        ``time_dropout`` the one it adds for every model whose name is not a FiLM one: accepted and unused, because
        reconstruction draws nothing and has no time embedding.  Any other keyword is a TypeError."""
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

    # ==================== Validation on the device ====================
    def _recon_pass(self, batches, keep: int = 0):
        """One pass over ``batches``: per batch ``decoder(encoder(x))`` and ONE ``spdm_recon_terms`` into the batch's slots of
        a float64 buffer sized for the pass; then one ``spdm_eval_reduce`` and ONE read-back.  Returns ``(val_loss, terms (N)
        on the device, the first `keep` frames, their reconstructions)``."""
        from .evaluation import reduce_errors
        from .train_metrics import recon_terms_into
        ids = getattr(batches, "row_ids", None)
        terms = torch.empty(max(len(ids) if ids is not None else 1024, 1), dtype=torch.float64, device=self.device)
        count, kept_x, kept_r = 0, [], []
        for batch in batches:
            x = batch.detach().to(self.device, torch.float32).contiguous()
            recon = self.decoder(self.encoder(x))
            n = x.shape[0]
            if count + n > terms.numel():       # a source of unknown length: the buffer grows on the device
                terms = torch.cat([terms, torch.empty(max(terms.numel(), count + n - terms.numel()), dtype=torch.float64, device=self.device)])
            recon_terms_into(recon, x, terms, count)
            if count < keep:
                kept_x.append(x[:keep - count]), kept_r.append(recon[:keep - count])
            count += n
        if count == 0:
            raise ValueError("validation_loss: no batches")
        terms = terms[:count]
        val_loss = float(reduce_errors(terms.view(count, 1), 1)[2].item())       # the one read-back
        return val_loss, terms, (torch.cat(kept_x) if kept_x else None), (torch.cat(kept_r) if kept_r else None)

    def validation_loss(self, batches, *, seed: int = 0, return_terms: bool = False):
        """The reference's ``val_loss`` (``validation_step`` over a ``val_dataloader()``, averaged by Lightning over the epoch
        with batch-size weights) formed on the device: every frame has 27648 elements, so it is the mean over the frames of
        each frame's own mean squared error (``spdm_recon_terms``, then ``spdm_eval_reduce``).  A Python float after ONE
        read-back; a deterministic function of the weights and the frames, whatever the batch size.  ``seed`` is ``train.fit``'s
        keyword and unused: nothing is drawn.  ``return_terms=True``: ``(val_loss, terms (N) float64 on the device)``."""
        val_loss, terms, _, _ = self._recon_pass(batches)
        return (val_loss, terms) if return_terms else val_loss

    def reconstruction_report(self, batches, *, sheet_frames: int = 8, cols: int = 8) -> dict:
        """What the reference's eval_autoencoder.py shows of a trained autoencoder, as numbers and one picture:
        ``{'val_loss', 'psnr_mean', 'psnr_min', 'worst', 'terms', 'sheet'}``.  ``terms`` (N) float64 on the host, the per-frame
        mean squared errors of ``validation_loss``; PSNR is ``10 log10(1 / mse)`` per frame in float64 on the host (``inf``
        for an exact reconstruction); ``worst``: the frames in descending order of error (the ``sheet_frames`` worst at most),
        as store rows when ``batches`` carries ``row_ids``, else as positions in the pass.  ``sheet``: a uint8 device tensor
        ``(2 ceil(k / cols) 96, cols 96, 3)`` from two ``spdm_frames_to_bytes`` launches, the first ``k = min(sheet_frames, N)``
        originals in the upper tiles and their reconstructions beneath (eval_autoencoder.py:91-106)."""
        from .dataset import frames_to_u8
        if sheet_frames < 1 or cols < 1:
            raise ValueError(f"sheet_frames = {sheet_frames} and cols = {cols} must be >= 1")
        val_loss, terms, x, recon = self._recon_pass(batches, keep=int(sheet_frames))
        k = x.shape[0]
        half = -(-k // cols) * cols                                  # tiles in the upper half: whole sheet rows
        sheet = torch.zeros((2 * half // cols * 96, cols * 96, 3), dtype=torch.uint8, device=self.device)
        frames_to_u8(x.contiguous(), sheet, cols=cols, tile_offset=0)
        frames_to_u8(recon.contiguous(), sheet, cols=cols, tile_offset=half)
        mse = terms.cpu().numpy()
        with np.errstate(divide="ignore"):
            psnr = 10.0 * np.log10(1.0 / mse)
        order = np.argsort(-mse, kind="stable")[:int(sheet_frames)]
        ids = getattr(batches, "row_ids", None)
        worst = [int(ids[i]) if ids is not None else int(i) for i in order]
        return {"val_loss": val_loss, "psnr_mean": float(psnr.mean()), "psnr_min": float(psnr.min()), "worst": worst,
                "terms": mse, "sheet": sheet}

    # ==================== Checkpoints (Lightning's layout; train_autoencoder.py's ModelCheckpoint) ====================
    def hparams(self) -> dict:
        """The constructor argument ``save_hyperparameters()`` records (models/encoder/autoencoder.py:44)."""
        return {"learning_rate": float(self.lr)}

    def save_hparams(self, path) -> None:
        import yaml
        with open(path, "w") as fh:
            fh.write(yaml.safe_dump(self.hparams(), sort_keys=False))

    def save_checkpoint(self, path, *, optimizer=None, scheduler=None, trainer_state: Optional[dict] = None) -> None:
        """Write ``path`` with ``torch.save`` in the layout of a Lightning checkpoint: ``state_dict`` (``self.state_dict()`` at
        the CURRENT values of both flat parameters), ``hyper_parameters``, ``epoch``, ``global_step``, ``optimizer_states``,
        ``lr_schedulers`` and the loop's counters under ``'spdm_trainer'``.  Host tensors only: the file holds nothing
        ``torch.load(weights_only=True)`` refuses, and ``load_from_checkpoint``, ``Diffusion_DDPM(vision_encoder_state_dict=
        safe_load_state_dict(path))`` and ``train --encoder_checkpoint path`` take it as it is."""
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

        ts = host(dict(trainer_state or {}))
        torch.save({"epoch": int(ts.get("epoch", 0)), "global_step": int(ts.get("global_step", 0)),
                    "pytorch-lightning_version": "2.0.0", "state_dict": self.state_dict(), "hyper_parameters": self.hparams(),
                    "optimizer_states": [host(optimizer.state_dict())] if optimizer is not None else [],
                    "lr_schedulers": [host(scheduler.state_dict())] if scheduler is not None else [],
                    "spdm_trainer": ts}, str(path))

    def restore_checkpoint(self, ckpt: dict) -> None:
        """Take both halves' tensors of a loaded checkpoint dict (``train.fit(ckpt_path=)``) into the existing handles and
        flat parameters in place: a configured optimiser keeps pointing at them."""
        sd = ckpt["state_dict"]
        enc_sd, dec_sd = encoder_state_dict_from(sd, "encoder."), decoder_state_dict_from(sd)
        if enc_sd is None or dec_sd is None:
            raise ValueError("the checkpoint's state_dict holds no autoencoder (encoder.N.* and decoder.N.*)")
        self.encoder.load_state_dict(enc_sd)
        self.decoder.load_state_dict(dec_sd)

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
