"""Train a noise predictor end to end: the counterpart of the reference's train.py.

    python -m state_policy_diffusionmodel_amd.train --arrays data.npz --model UNet_FilmnoAttention --n_epochs 50 --out_dir run0

``fit`` restates what train.py asks of Lightning's Trainer -- ``max_epochs``, ``val_check_interval=0.25``,
``gradient_clip_val=0.5``, ``ModelCheckpoint(filename='{epoch}', save_top_k=-1, every_n_epochs=1)``,
``EarlyStopping(monitor='lr', ...)``, ``ReduceLROnPlateau`` on ``val_loss``, ``trainer.validate`` before ``trainer.fit`` and the
``STATS.pkl`` written between the two -- as one plain loop over this project's device-side pieces: batches assembled in HBM
(dataset.py), the noising process in one launch, loss, gradients, clipping and Adam in HIP (``training_step`` /
``optimizer_step``), and a validation pass that stays on the device (``validation_loss``).  The loop reads nothing back per
step: each step's loss scalar is copied into a device ring that is fetched once per validation and at the end of an epoch.

The model and the data module are duck-typed (the methods used are listed at ``fit``), so the loop itself runs on the CPU
with stubs; with the real objects there is no CPU fallback.  Lightning is not a dependency and the restatement was not
checked against it; what it does NOT restate is listed in DESIGN.md 8.12."""
from __future__ import annotations

import argparse
import json
import os
from typing import Optional

import numpy as np
import torch

from .weights import is_simple_model


class LrEarlyStop:
    """train.py's ``EarlyStopping(monitor='lr', stopping_threshold=threshold, patience=patience)`` (mode 'min'), checked
    after every validation on the optimiser's current learning rate: stop if ``lr < threshold`` (strictly); otherwise a
    validation at which the lr is lower than at any before resets the count, any other adds one, and the run stops when the
    count reaches ``patience``."""

    def __init__(self, threshold: float = 1e-4, patience: int = 50):
        self.threshold, self.patience = float(threshold), int(patience)
        self.best = float("inf")
        self.wait = 0
        self.reason: Optional[str] = None

    def check(self, lr: float) -> bool:
        lr = float(lr)
        if lr < self.threshold:
            self.reason = f"lr {lr:g} < stopping_threshold {self.threshold:g}"
            return True
        if lr < self.best:
            self.best, self.wait = lr, 0
            return False
        self.wait += 1
        if self.wait >= self.patience:
            self.reason = f"lr did not decrease in {self.wait} validations (patience {self.patience})"
            return True
        return False

    def state_dict(self) -> dict:
        return {"threshold": self.threshold, "patience": self.patience, "best": self.best, "wait": self.wait}

    def load_state_dict(self, sd: dict) -> None:
        self.best, self.wait = float(sd["best"]), int(sd["wait"])


def validation_points(n_train_batches: int, val_check_interval=0.25):
    """The 0-based train batch indices of an epoch after which validation runs: a float is a fraction of the epoch
    (``(i + 1) % max(1, int(n_train_batches * val_check_interval)) == 0``), an int a number of batches."""
    if isinstance(val_check_interval, int) and not isinstance(val_check_interval, bool):
        every = max(1, val_check_interval)
    else:
        if not 0.0 < float(val_check_interval) <= 1.0:
            raise ValueError(f"val_check_interval = {val_check_interval} must lie in (0, 1] (or be a number of batches)")
        every = max(1, int(n_train_batches * float(val_check_interval)))
    return [i for i in range(n_train_batches) if (i + 1) % every == 0]


def _lr(optimizer) -> float:
    return float(optimizer.param_groups[0]["lr"])


def fit(model, datamodule, *, max_epochs: int, out_dir, val_check_interval=0.25, gradient_clip_val: Optional[float] = 0.5,
        seed: int = 0, device_optimizer: bool = True, early_stop: Optional[LrEarlyStop] = None, ckpt_path=None,
        validate_first: bool = True, log_every: int = 0, ema: Optional[dict] = None, ema_monitor: bool = False) -> dict:
    """Train ``model`` on ``datamodule`` for epochs ``[start, max_epochs)`` and write ``out_dir/checkpoints/epoch={e}.ckpt``
    (every epoch, all kept), ``out_dir/STATS.pkl``, ``out_dir/hparams.yaml`` and ``out_dir/metrics.jsonl``.

    Used of ``model``: ``configure_optimizers(device_optimizer=)``, ``training_step(batch, backward=True, device_noise=True,
    seed=, noise_step=[, time_dropout=0.1 for model='UNet'])`` returning a loss scalar tensor, ``optimizer_step(optimizer,
    gradient_clip_val)``, ``validation_loss(batches, seed=)`` returning a float, ``save_checkpoint``, ``save_hparams``,
    ``restore_checkpoint(ckpt)`` (resume only), and the attributes ``model_name`` and ``device``.  Of ``datamodule``:
    ``train_dataloader(epoch)`` (sized, iterable), ``val_dataloader()`` and, when it has one, ``save_stats(path)`` (no
    ``STATS.pkl`` otherwise).

    A step is ``training_step`` then ``optimizer_step``; training step ``g`` (counted over the whole run) draws its noise from
    ``(seed, g)``, epoch ``e`` its order from the data module's ``(seed, e)``.  Validation runs after the train batches
    ``validation_points`` names, on ``validation_loss(datamodule.val_dataloader(), seed=seed)``; ``early_stop`` is checked
    after each on the current lr; when it fires the epoch ends there (scheduler step, checkpoint and log line included) and
    the run stops.  At the end of an epoch ``scheduler.step(latest val_loss)``.  ``validate_first``: one validation pass
    before training (not on resume), as the reference's ``trainer.validate``.  ``ckpt_path``: a checkpoint of this loop;
    weights, optimiser, scheduler, counters, the latest val_loss and the early-stop state are restored and training goes on
    at the next epoch, appending to ``metrics.jsonl``.  ``log_every`` > 0 prints every that many steps (no read-back: the
    step number only); validation lines are always printed.

    ``ema`` (a dict of ``optim.ema_decay``'s schedule keywords, ``{}`` for its defaults): the loop calls
    ``model.configure_ema(**ema)`` once -- ``optimizer_step`` then keeps the average -- and every validation also computes
    ``val_loss_ema = validation_loss(..., use_ema=True)``; every ``metrics.jsonl`` line gains ``val_loss_ema`` and ``ema_decay``
    (the decay of the latest update).  The scheduler, and through its lr the early stop, keep following ``val_loss`` unless
    ``ema_monitor`` makes them follow ``val_loss_ema``.  A resumed run restores the shadow and its counter
    (``restore_checkpoint``).  ``None``: none of this; ``configure_ema`` is not looked up.

    Returns ``{'epoch', 'global_step', 'val_loss', 'lr', 'stopped_early', 'metrics'}`` (and ``'val_loss_ema'`` with ``ema``)."""
    out_dir = str(out_dir)
    ckpt_dir = os.path.join(out_dir, "checkpoints")
    os.makedirs(ckpt_dir, exist_ok=True)
    if hasattr(model, "_max_batch") and hasattr(datamodule, "batch_size"):     # engines are built for the full batch first
        model._max_batch = max(int(model._max_batch), int(datamodule.batch_size))
    conf = model.configure_optimizers(device_optimizer=device_optimizer)
    optimizer, scheduler = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    step_kw = {"time_dropout": 0.1} if is_simple_model(getattr(model, "model_name", "UNet_Film")) else {}
    device = getattr(model, "device", "cpu")
    if ema_monitor and ema is None:
        raise ValueError("ema_monitor=True needs ema= (there is no val_loss_ema to follow)")
    ema_obj = model.configure_ema(**ema) if ema is not None else None
    val_loss_ema = None

    start_epoch, global_step, val_loss = 0, 0, None
    if ckpt_path is not None:
        ckpt = torch.load(str(ckpt_path), map_location="cpu", weights_only=True)
        st = ckpt.get("spdm_trainer")
        if not isinstance(st, dict) or "epoch" not in st:
            raise ValueError(f"{ckpt_path} holds no 'spdm_trainer' state: it was not written by this loop")
        model.restore_checkpoint(ckpt)
        optimizer.load_state_dict(ckpt["optimizer_states"][0])
        scheduler.load_state_dict(ckpt["lr_schedulers"][0])
        start_epoch, global_step, val_loss = int(st["epoch"]) + 1, int(st["global_step"]), st.get("val_loss")
        val_loss_ema = st.get("val_loss_ema")
        if int(st.get("seed", seed)) != int(seed):
            raise ValueError(f"{ckpt_path} was trained with seed {st['seed']}, this call has seed {seed}")
        if early_stop is not None and st.get("early_stop"):
            early_stop.load_state_dict(st["early_stop"])

    metrics = []
    log = open(os.path.join(out_dir, "metrics.jsonl"), "a" if ckpt_path is not None else "w")

    def emit(kind, epoch, train_loss):
        line = {"kind": kind, "epoch": epoch, "global_step": global_step, "val_loss": val_loss, "lr": _lr(optimizer),
                "train_loss": train_loss}
        if ema is not None:
            from .optim import ema_decay
            line["val_loss_ema"] = val_loss_ema
            line["ema_decay"] = ema_decay(int(getattr(ema_obj, "optimization_step", global_step)), **ema)
        metrics.append(line)
        log.write(json.dumps(line) + "\n")
        log.flush()
        print(f"[{kind}] epoch {epoch} step {global_step} val_loss {val_loss} lr {line['lr']:g} train_loss {train_loss}", flush=True)

    def validate():
        nonlocal val_loss, val_loss_ema
        val_loss = float(model.validation_loss(datamodule.val_dataloader(), seed=seed))
        if ema is not None:
            val_loss_ema = float(model.validation_loss(datamodule.val_dataloader(), seed=seed, use_ema=True))

    try:
        if ckpt_path is None:
            if validate_first:
                validate()
                emit("val", -1, None)
            if hasattr(datamodule, "save_stats"):       # (the frame autoencoder's data has no statistics, as in the reference)
                datamodule.save_stats(os.path.join(out_dir, "STATS.pkl"))
            model.save_hparams(os.path.join(out_dir, "hparams.yaml"))

        ring = None
        stopped = False
        epoch = start_epoch - 1
        for epoch in range(start_epoch, int(max_epochs)):
            loader = datamodule.train_dataloader(epoch)
            n = len(loader)
            points = set(validation_points(n, val_check_interval))
            if ring is None or ring.numel() < n:
                ring = torch.zeros(max(n, 1), dtype=torch.float32, device=device)
            filled = 0

            def drain():
                """mean of the ring's entries since the last line (float64 on the host): the one read-back of the losses"""
                nonlocal filled
                if filled == 0:
                    return None
                vals = np.asarray(ring[:filled].tolist(), dtype=np.float64)
                filled = 0
                return float(vals.mean())

            for i, batch in enumerate(loader):
                loss = model.training_step(batch, backward=True, device_noise=True, seed=seed, noise_step=global_step, **step_kw)
                model.optimizer_step(optimizer, gradient_clip_val)
                ring[filled].copy_(loss)
                filled += 1
                global_step += 1
                if log_every and global_step % log_every == 0:
                    print(f"epoch {epoch} batch {i + 1}/{n} step {global_step}", flush=True)
                if i in points:
                    validate()
                    emit("val", epoch, drain())
                    if early_stop is not None and early_stop.check(_lr(optimizer)):
                        stopped = True
                        break
            monitored = val_loss_ema if ema_monitor else val_loss
            if monitored is not None:
                scheduler.step(monitored)
            emit("epoch", epoch, drain())
            state = {"epoch": epoch, "global_step": global_step, "val_loss": val_loss, "seed": int(seed),
                     "early_stop": early_stop.state_dict() if early_stop is not None else None, "stopped_early": stopped}
            if ema is not None:
                state["val_loss_ema"] = val_loss_ema
            model.save_checkpoint(os.path.join(ckpt_dir, f"epoch={epoch}.ckpt"), optimizer=optimizer, scheduler=scheduler,
                                  trainer_state=state)
            if stopped:
                print(f"early stop: {early_stop.reason}", flush=True)
                break
    finally:
        log.close()
    result = {"epoch": epoch, "global_step": global_step, "val_loss": val_loss, "lr": _lr(optimizer), "stopped_early": stopped,
              "metrics": metrics}
    if ema is not None:
        result["val_loss_ema"] = val_loss_ema
    return result


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m state_policy_diffusionmodel_amd.train", description="Training script")
    p.add_argument("--n_epochs", type=int, default=500, help="Number of epochs")
    p.add_argument("--amp", action="store_true", help="(refused: training here is exact fp32)")
    p.add_argument("--batch_size", type=int, default=16, help="Batch size")
    p.add_argument("--lr", type=float, default=1e-4, help="Learning rate")
    p.add_argument("--obs_horizon", type=int, default=10)
    p.add_argument("--pred_horizon", type=int, default=30)
    p.add_argument("--action_horizon", type=int, default=1, help="(accepted for the reference's command lines; unused, as there)")
    p.add_argument("--inpaint_horizon", type=int, default=1)
    p.add_argument("--step_size", type=int, default=5, help="Rate of sampling from the dataset")
    p.add_argument("--noise_steps", type=int, default=1000, help="Denoising steps")
    p.add_argument("--cond_dim", type=int, default=128 + 2 + 3 + 2, help="Dimension of one observation row")
    p.add_argument("--output_dim", type=int, default=5, help="Dimension of one predicted row")
    p.add_argument("--model", type=str, default="UNet_Film", help="UNet_Film, UNet_FilmnoAttention or UNet")
    p.add_argument("--noise_scheduler", type=str, default="linear")
    p.add_argument("--dataset_dir", type=str, default="./data")
    p.add_argument("--dataset", type=str, default=None, help="zarr store under --dataset_dir (needs the zarr package)")
    p.add_argument("--arrays", type=str, default=None, help=".npz with position, velocity, action, img, episode_ends (instead of --dataset)")
    p.add_argument("--encoder_checkpoint", type=str, default=None,
                   help="state_dict file of the frame encoder (or a checkpoint holding vision_encoder.* entries)")
    p.add_argument("--out_dir", type=str, default="runs/train")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--no_early_stop", action="store_true")
    p.add_argument("--ckpt_path", type=str, default=None, help="resume from a checkpoint of this loop")
    p.add_argument("--ema", action="store_true", help="keep an exponential moving average of the weights (DESIGN.md 8.22)")
    p.add_argument("--ema_max_decay", type=float, default=0.9999, help="the decay the warm-up schedule ends at")
    p.add_argument("--ema_power", type=float, default=0.75, help="exponent of the warm-up schedule")
    p.add_argument("--ema_inv_gamma", type=float, default=1.0, help="inverse multiplicative factor of the warm-up schedule")
    p.add_argument("--ema_update_after_step", type=int, default=0, help="optimiser steps before the average starts to lag")
    p.add_argument("--ema_monitor", action="store_true", help="the lr scheduler follows val_loss_ema instead of val_loss")
    return p


def main(argv=None) -> dict:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.amp:
        parser.error("--amp is not supported: training here runs on the exact fp32 MFMA path (there is no mixed-precision "
                     "training pass); drop the flag")
    if (args.dataset is None) == (args.arrays is None):
        parser.error("pass exactly one of --dataset (a zarr store) and --arrays (an .npz file)")
    from .dataset import CarRacingDataModule
    from .diffusion import Diffusion_DDPM
    dm = CarRacingDataModule(args.batch_size, args.dataset_dir, args.obs_horizon, args.pred_horizon, seed=args.seed,
                             step_size=args.step_size)
    if args.arrays is not None:
        with np.load(args.arrays) as z:
            dm.setup(arrays={k: z[k] for k in ("position", "velocity", "action", "img", "episode_ends")})
    else:
        dm.setup(name=args.dataset)
    enc_sd = None
    if args.encoder_checkpoint is not None:
        from .weights import safe_load_state_dict
        enc_sd = safe_load_state_dict(args.encoder_checkpoint)
    kw = dict(noise_steps=args.noise_steps, obs_horizon=args.obs_horizon, pred_horizon=args.pred_horizon,
              observation_dim=args.cond_dim, prediction_dim=args.output_dim, model=args.model, learning_rate=args.lr,
              inpaint_horizon=args.inpaint_horizon, noise_scheduler_type=args.noise_scheduler, step_size=args.step_size,
              max_batch=args.batch_size, train_attention=args.model == "UNet_Film")
    if enc_sd is not None:
        kw["vision_encoder_state_dict"] = enc_sd
    if args.ckpt_path is not None:
        model = Diffusion_DDPM.load_from_checkpoint(args.ckpt_path, **kw)
    else:
        model = Diffusion_DDPM(weight_seed=args.seed, **kw)
    early = None if args.no_early_stop else LrEarlyStop(1e-4, args.n_epochs // 10)
    extra = {}
    if args.ema:
        extra = {"ema": {"max_value": args.ema_max_decay, "power": args.ema_power, "inv_gamma": args.ema_inv_gamma,
                         "update_after_step": args.ema_update_after_step}, "ema_monitor": args.ema_monitor}
    elif args.ema_monitor:
        parser.error("--ema_monitor needs --ema")
    return fit(model, dm, max_epochs=args.n_epochs, out_dir=args.out_dir, seed=args.seed, early_stop=early,
               ckpt_path=args.ckpt_path, log_every=50, **extra)


__all__ = ["LrEarlyStop", "validation_points", "fit", "main", "build_parser"]

if __name__ == "__main__":
    main()
