"""Train the frame autoencoder end to end: the counterpart of the reference's models/encoder/train_autoencoder.py
(DESIGN.md 8.23).

    python -m state_policy_diffusionmodel_amd.train_autoencoder --arrays data.npz --n_epochs 50 --out_dir runs/autoencoder

The run is ``train.fit`` -- the loop that trains the noise predictor -- with the reference's Trainer settings for this stage
(train_autoencoder.py:76-89): ``val_check_interval=0.5``, ``gradient_clip_val=0.5``, ``EarlyStopping(monitor='lr',
stopping_threshold=2e-6, patience=n_epochs)``, ``ModelCheckpoint(filename='{epoch}', save_top_k=-1)``.  Frames come from a
``FramesDataModule`` (the frames stay in HBM), every step is ``autoencoder.training_step(backward=True)`` +
``optimizer_step`` in HIP, validation is ``autoencoder.validation_loss`` on the device.  It leaves
``out_dir/checkpoints/epoch={e}.ckpt``, ``hparams.yaml`` and ``metrics.jsonl``; a checkpoint is what ``train
--encoder_checkpoint`` takes.  There is no CPU fallback."""
from __future__ import annotations

import argparse

import numpy as np

from .train import LrEarlyStop, fit

VAL_CHECK_INTERVAL, GRADIENT_CLIP_VAL, LR_STOPPING_THRESHOLD = 0.5, 0.5, 2e-6     # train_autoencoder.py:76-89


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m state_policy_diffusionmodel_amd.train_autoencoder",
                                description="Train the frame autoencoder")
    p.add_argument("--arrays", type=str, default=None, help=".npz with img (T,96,96,3); one written for train --arrays works as it is")
    p.add_argument("--dataset", type=str, default=None, help="zarr store under --dataset_dir (needs the zarr package)")
    p.add_argument("--dataset_dir", type=str, default="./data")
    p.add_argument("--batch_size", type=int, default=128, help="Batch size")
    p.add_argument("--n_epochs", type=int, default=50, help="Number of epochs")
    p.add_argument("--lr", type=float, default=1e-3, help="Learning rate")
    p.add_argument("--out_dir", type=str, default="runs/autoencoder")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--ckpt_path", type=str, default=None, help="resume from a checkpoint of this loop")
    p.add_argument("--no_early_stop", action="store_true")
    p.add_argument("--image_storage", type=str, default="auto", choices=("auto", "uint8", "float32"))
    return p


def main(argv=None) -> dict:
    parser = build_parser()
    args = parser.parse_args(argv)
    if (args.dataset is None) == (args.arrays is None):
        parser.error("pass exactly one of --dataset (a zarr store) and --arrays (an .npz file)")
    from .autoencoder import autoencoder
    from .dataset import FramesDataModule
    dm = FramesDataModule(args.batch_size, args.dataset_dir, seed=args.seed, image_storage=args.image_storage)
    if args.arrays is not None:
        with np.load(args.arrays) as z:
            dm.setup(arrays={"img": z["img"]})
    else:
        dm.setup(name=args.dataset)
    if args.ckpt_path is not None:
        model = autoencoder.load_from_checkpoint(args.ckpt_path, learning_rate=args.lr)
    else:
        model = autoencoder(learning_rate=args.lr, weight_seed=args.seed)
    early = None if args.no_early_stop else LrEarlyStop(LR_STOPPING_THRESHOLD, args.n_epochs)
    return fit(model, dm, max_epochs=args.n_epochs, out_dir=args.out_dir, val_check_interval=VAL_CHECK_INTERVAL,
               gradient_clip_val=GRADIENT_CLIP_VAL, seed=args.seed, early_stop=early, validate_first=True, device_optimizer=True,
               ckpt_path=args.ckpt_path, log_every=50)


__all__ = ["build_parser", "main"]

if __name__ == "__main__":
    main()
