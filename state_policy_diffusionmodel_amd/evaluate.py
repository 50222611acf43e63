"""CLI of ``evaluation.evaluate``: the question the reference's evaluation/eval_acurracy_diffusion_positions.py and
eval_consistency_diffusion_positions.py ask of a trained model -- how far are its predicted positions from the truth? --
answered for every window of a dataset, ``--runs`` times each, on the device.

    python -m state_policy_diffusionmodel_amd.evaluate --model_name DDIM --checkpoint epoch=39.ckpt --hparams hparams.yaml \\
        --stats STATS.pkl --data arrays.npz --runs 10 --out report.json

``--data`` is an ``.npz`` with ``position`` (T,2), ``velocity`` (T,2), ``action`` (T,3), ``img`` (T,96,96,3) and
``episode_ends``; any other path is opened as a zarr store with the reference's layout, which needs the zarr package and is
NOT covered by the tests.  ``--stats`` is the ``[stats]`` pickle the training run saved (``CarRacingDataModule.save_stats``,
utils/data_utils.py:42-44); it is read by an unpickler that admits numpy arrays and plain containers only.  Without it the
statistics are computed from the data.

``--noise_levels 0,0.01,0.05`` also asks the question of evaluation/eval_robustness.py -- how much worse does the prediction get
when the observations are noisy? -- with ``evaluation.robustness`` at ``--runs`` runs per window, and writes its report under
``"robustness"`` in the JSON.  Without the flag the output is what it was."""
from __future__ import annotations

import argparse
import json
import pickle
import time

import numpy as np

_NUMPY_GLOBALS = {(m, n) for m in ("numpy", "numpy.core.multiarray", "numpy._core.multiarray", "numpy.core.numeric", "numpy._core.numeric")
                  for n in ("_reconstruct", "ndarray", "dtype", "scalar", "_frombuffer")}


class _StatsUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) in _NUMPY_GLOBALS:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"{module}.{name} is not part of a statistics file")


def load_stats(path: str) -> dict:
    with open(path, "rb") as f:
        stats = _StatsUnpickler(f).load()
    stats = stats[0] if isinstance(stats, (list, tuple)) else stats
    if not isinstance(stats, dict) or not {"position", "velocity", "action"} <= set(stats):
        raise ValueError(f"{path}: expected [{{'position', 'velocity', 'action'}}] statistics")
    return stats


def load_arrays(path: str) -> dict:
    keys = ("position", "velocity", "action", "img")
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {**{k: z[k] for k in keys}, "episode_ends": z["episode_ends"]}
    try:
        import zarr
    except ImportError as e:
        raise ImportError(f"{path} is not an .npz file; reading it as a zarr store needs the zarr package") from e
    root = zarr.open(path, "r")
    return {**{k: root["data"][k][:] for k in keys}, "episode_ends": root["meta"]["episode_ends"][:]}


def parse_arguments(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model_name", type=str, default="DDIM", choices=("DDPM", "DDIM"))
    p.add_argument("--checkpoint", type=str, required=True, help="state_dict file with noise_estimator.* (and vision_encoder.*) tensors")
    p.add_argument("--hparams", type=str, required=True, help="hparams.yaml written next to the checkpoint")
    p.add_argument("--stats", type=str, default=None, help="STATS.pkl of the training run (default: computed from --data)")
    p.add_argument("--data", type=str, required=True, help="arrays.npz (or a zarr store, if zarr is installed)")
    p.add_argument("--ddim_steps", type=int, default=100)
    p.add_argument("--solver_steps", type=int, default=None, metavar="N", help="sample with DPM-Solver++ (2M) in N steps instead of the --model_name schedule (default: off)")
    p.add_argument("--use_ema", action="store_true", help="load the checkpoint's averaged weights (ema_state_dict, written by train --ema)")
    p.add_argument("--step_size", type=int, default=None, help="rows between a window's samples (default: the hparams' step_size)")
    p.add_argument("--runs", type=int, default=10)
    p.add_argument("--batch_size", type=int, default=4096)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--no_actions", action="store_true", help="position error only")
    p.add_argument("--noise_levels", type=str, default=None, help="comma-separated alphas: also measure the error under alpha * U[0,1) "
                                                                    "added to the observations (evaluation.robustness)")
    p.add_argument("--out", type=str, default=None, help="report.json")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_arguments(argv)
    from .dataset import DeviceDataset
    from .diffusion import load_model
    from .evaluation import evaluate, robustness
    from .weights import fetch_hyperparams_from_yaml
    model = load_model(args.model_name, args.checkpoint, args.hparams, num_of_ddim_steps=args.ddim_steps, max_batch=args.batch_size,
                       solver_steps=args.solver_steps, use_ema=args.use_ema)
    step_size = int(args.step_size or dict(fetch_hyperparams_from_yaml(args.hparams)).get("step_size", 1))
    arrays = load_arrays(args.data)
    dataset = DeviceDataset(arrays["position"], arrays["velocity"], arrays["action"], arrays["img"], arrays["episode_ends"],
                            model.pred_horizon, model.obs_horizon, step_size=step_size,
                            stats=load_stats(args.stats) if args.stats else None, device=model.device.index)
    start = time.time()
    report = evaluate(model, dataset, runs=args.runs, batch_size=args.batch_size, seed=args.seed, actions=not args.no_actions)
    print(f"*** {len(dataset)} windows x {args.runs} runs in {time.time() - start:.2f} s")
    print("mean position error per step:", np.array2string(report.mean_error, precision=4))
    print("std  position error per step:", np.array2string(report.std_error, precision=4))
    robust = None
    if args.noise_levels is not None:
        levels = [float(v) for v in args.noise_levels.split(",")]
        start = time.time()
        robust = robustness(model, dataset, levels=levels, runs=args.runs, batch_size=args.batch_size, seed=args.seed)
        print(f"*** {len(levels)} noise levels in {time.time() - start:.2f} s")
        for name in ("mse_position", "mse_action"):
            print(f"{name} per level:", np.array2string(getattr(robust, name), precision=6))
    if args.out:
        with open(args.out, "w") as f:
            f.write(report.to_json() if robust is None else json.dumps({**report.to_dict(), "robustness": robust.to_dict()}))
    return report


if __name__ == "__main__":
    main()
