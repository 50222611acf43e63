"""Look at a trained frame autoencoder: the counterpart of the reference's models/encoder/eval_autoencoder.py.

    python -m state_policy_diffusionmodel_amd.eval_autoencoder --checkpoint runs/autoencoder/checkpoints/epoch=49.ckpt \\
        --arrays data.npz --out report.json --sheet sheet.ppm

Runs ``autoencoder.reconstruction_report`` over the validation split (or every frame) and writes the numbers as JSON and
the originals-over-reconstructions contact sheet as a binary PPM, which needs no image library.  The split is
``FramesDataModule``'s: the one the run with the same non-zero ``--seed`` validated on (``split_indices`` takes seed 0, as every
falsy seed, for torch's default generator, like the reference: that split is not reproducible).  There is no CPU fallback."""
from __future__ import annotations

import argparse
import json

import numpy as np


def write_ppm(path, pixels) -> None:
    """``pixels`` (H, W, 3) uint8 as a binary PPM: the header ``P6\\nW H\\n255\\n``, then the bytes row by row, R G B."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 3:
        raise ValueError(f"expected (H, W, 3) uint8 pixels, got {pixels.shape} {pixels.dtype}")
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (pixels.shape[1], pixels.shape[0]))
        fh.write(pixels.tobytes())


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m state_policy_diffusionmodel_amd.eval_autoencoder",
                                description="Reconstruction error and a contact sheet of a trained frame autoencoder")
    p.add_argument("--checkpoint", type=str, required=True, help="a checkpoint of train_autoencoder (or of the reference's run)")
    p.add_argument("--arrays", type=str, default=None, help=".npz with img (T,96,96,3)")
    p.add_argument("--dataset", type=str, default=None, help="zarr store under --dataset_dir (needs the zarr package)")
    p.add_argument("--dataset_dir", type=str, default="./data")
    p.add_argument("--split", type=str, default="val", choices=("val", "all"))
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--seed", type=int, default=0, help="the run's seed: non-zero, it decides the validation split (0: torch's default generator)")
    p.add_argument("--out", type=str, default=None, help="write the report as JSON here")
    p.add_argument("--terms", action="store_true", help="include every frame's mean squared error in the JSON")
    p.add_argument("--sheet", type=str, default=None, help="write the contact sheet as a binary PPM here")
    p.add_argument("--sheet_frames", type=int, default=8)
    p.add_argument("--columns", type=int, default=8)
    p.add_argument("--image_storage", type=str, default="auto", choices=("auto", "uint8", "float32"))
    return p


def main(argv=None) -> dict:
    parser = build_parser()
    args = parser.parse_args(argv)
    if (args.dataset is None) == (args.arrays is None):
        parser.error("pass exactly one of --dataset (a zarr store) and --arrays (an .npz file)")
    from .autoencoder import autoencoder
    from .dataset import FramesDataModule, _FrameBatches
    dm = FramesDataModule(args.batch_size, args.dataset_dir, seed=args.seed, image_storage=args.image_storage)
    if args.arrays is not None:
        with np.load(args.arrays) as z:
            dm.setup(arrays={"img": z["img"]})
    else:
        dm.setup(name=args.dataset)
    batches = dm.val_dataloader() if args.split == "val" else _FrameBatches(dm.data_full, np.arange(len(dm.data_full)), args.batch_size)
    model = autoencoder.load_from_checkpoint(args.checkpoint)
    rep = model.reconstruction_report(batches, sheet_frames=args.sheet_frames, cols=args.columns)
    out = {"checkpoint": args.checkpoint, "split": args.split, "frames": int(rep["terms"].size), "val_loss": rep["val_loss"],
           "psnr_mean": rep["psnr_mean"], "psnr_min": rep["psnr_min"], "worst": rep["worst"]}
    if args.terms:
        out["terms"] = rep["terms"].tolist()
    if args.out is not None:
        with open(args.out, "w") as fh:
            json.dump(out, fh)
            fh.write("\n")
    if args.sheet is not None:
        write_ppm(args.sheet, rep["sheet"].cpu().numpy())
    print(json.dumps({k: v for k, v in out.items() if k != "terms"}), flush=True)
    out["sheet"] = rep["sheet"]
    return out


__all__ = ["build_parser", "main", "write_ppm"]

if __name__ == "__main__":
    main()
