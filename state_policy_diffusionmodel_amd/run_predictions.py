"""CLI of ``policy.ClosedLoopPolicy``: the loop of the reference's run_predictions.py:112-175 replayed over recorded episodes.

    python -m state_policy_diffusionmodel_amd.run_predictions --model_name DDIM --checkpoint epoch=39.ckpt --hparams hparams.yaml \\
        --stats STATS.pkl --data arrays.npz --replan_every 50 --seed 0 --out report.json

The reference drives its simulator (gym 0.21 / Box2D), which this project does not ship; the recorded episodes of ``--data``
(the ``.npz`` / zarr layout of ``evaluate``) stand in for it.  Per episode: ``reset()``, then ``observe()`` row by row, and a
``plan()`` on every ``--replan_every``-th row of the episode (:151).  Way-point j of a plan made at row t lies ``(j + 1)
step_size`` rows after the newest observation's window slot, at row ``t - step_size + 1 + (j + 1) step_size`` -- the row a
dataset window starting at ``t - L + 1`` predicts at step j -- and is compared with the recorded position there by the 2-norm
in float64.  Steps past the episode's end are left out and counted.

The report holds per plan its row, its errors and the wall-clock seconds of ``plan()`` (synchronised), and over all plans the
mean and population std of the error per step.

``--warm_start K`` replans inside an episode from the previous plan with the last K denoise steps only (``plan(warm_start=K)``,
DESIGN.md 8.18); the first plan of every episode is cold, because the policy is reset there.  Each plan then also says how many
steps it ran and whether it was warm, and the report holds the error statistics and the mean seconds of the cold and of the warm
plans side by side -- what a checkpoint's owner needs to choose K.

``--candidates K`` samples K candidates per plan and keeps one, chosen on the device (``plan_candidates(candidates=K,
select=..., cols=...)``).  Each plan then also holds ``chosen``, ``selected_by``, the chosen candidate's ``score`` (what it was
``scored_by``, over how many ``rows``) and the per-step ``spread`` of the candidates; the report holds ``mean_spread`` per step and
``mean_jump``: the mean, over the plans scored against their predecessor, of the chosen candidate's coherence score divided by
``rows x cols`` -- the mean squared step between consecutive plans, in normalised units.  ``--select first`` keeps candidate 0 and
reports the same numbers for it, so that two runs compare."""
from __future__ import annotations

import argparse
import json
import time
from typing import List, Tuple

import numpy as np


def plan_rows(t: int, first: int, end: int, obs_horizon: int, pred_horizon: int, step_size: int) -> Tuple[List[int], List[int], int]:
    """The store rows a plan made after observing row ``t`` of the episode ``[first, end)`` involves: ``(observed, predicted,
    left_out)``.  ``observed``: the rows of the ``obs_horizon`` history entries, oldest first -- ``t - L + 1 + k step_size``
    with ``L = obs_horizon step_size``, or ``first`` where the history still holds the initial fill.  ``predicted``: the rows
    ``t - step_size + 1 + (j + 1) step_size`` of the way-points ``j < pred_horizon`` that lie before ``end``; ``left_out``: how
    many do not."""
    if not first <= t < end:
        raise ValueError(f"row {t} outside the episode [{first}, {end})")
    if obs_horizon < 1 or pred_horizon < 1 or step_size < 1:
        raise ValueError("obs_horizon, pred_horizon and step_size must be >= 1")
    L = obs_horizon * step_size
    observed = [max(first, t - L + 1 + k * step_size) for k in range(obs_horizon)]
    rows = [t - step_size + 1 + (j + 1) * step_size for j in range(pred_horizon)]
    predicted = [r for r in rows if r < end]
    return observed, predicted, len(rows) - len(predicted)


def parse_arguments(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model_name", type=str, default="DDIM", choices=("DDPM", "DDIM"))
    p.add_argument("--checkpoint", type=str, required=True, help="state_dict file with noise_estimator.* (and vision_encoder.*) tensors")
    p.add_argument("--hparams", type=str, required=True, help="hparams.yaml written next to the checkpoint")
    p.add_argument("--stats", type=str, required=True, help="STATS.pkl of the training run")
    p.add_argument("--data", type=str, required=True, help="arrays.npz (or a zarr store, if zarr is installed)")
    p.add_argument("--ddim_steps", type=int, default=100)
    p.add_argument("--solver_steps", type=int, default=None, metavar="N", help="sample with DPM-Solver++ (2M) in N steps instead of the --model_name schedule (default: off)")
    p.add_argument("--use_ema", action="store_true", help="load the checkpoint's averaged weights (ema_state_dict, written by train --ema)")
    p.add_argument("--replan_every", type=int, default=50, help="plan on every n-th row of an episode (run_predictions.py:151)")
    p.add_argument("--seed", type=int, default=0, help="plan i samples with seed + i and its x_T from a generator seeded alike")
    p.add_argument("--warm_start", type=int, default=None, metavar="K",
                   help="replan inside an episode from the previous plan, running the last K denoise steps only (default: off)")
    p.add_argument("--candidates", type=int, default=1, metavar="K", help="sample K candidates per plan and keep one (default: 1, off)")
    p.add_argument("--select", type=str, default="coherent", choices=("coherent", "medoid", "first"),
                   help="with --candidates: closest to the previous plan (medoid when there is none), the medoid, or candidate 0")
    p.add_argument("--select_cols", type=int, default=2, metavar="C", help="columns of a row that enter a distance: 2 positions, 5 with actions")
    p.add_argument("--out", type=str, default=None, help="report.json")
    return p.parse_args(argv)


def main(argv=None) -> dict:
    args = parse_arguments(argv)
    if args.replan_every < 1:
        raise SystemExit("--replan_every must be >= 1")
    if args.warm_start is not None and args.warm_start < 1:
        raise SystemExit("--warm_start must be >= 1")
    if not 1 <= args.candidates <= 64:
        raise SystemExit("--candidates must be in [1, 64]")
    import torch
    from .dataset import choose_image_storage
    from .diffusion import load_model
    from .evaluate import load_arrays, load_stats
    from .policy import ClosedLoopPolicy
    model = load_model(args.model_name, args.checkpoint, args.hparams, num_of_ddim_steps=args.ddim_steps, max_batch=args.candidates,
                       solver_steps=args.solver_steps, use_ema=args.use_ema)
    stats = load_stats(args.stats)
    arrays = load_arrays(args.data)
    storage = choose_image_storage(arrays["img"])
    policy = ClosedLoopPolicy(model, stats, n_envs=1, image_storage=storage, device=model.device.index)
    obs_h, P, s = policy.obs_horizon, policy.pred_horizon, policy.step_size
    H, D = P + policy.inpaint_horizon, policy.prediction_dim
    position = np.asarray(arrays["position"], dtype=np.float64)
    u8 = storage == "uint8"
    K = args.candidates
    many = {"candidates": K, "select": args.select, "cols": args.select_cols} if K > 1 else {}     # 1: the calls of before
    plans, left_out, first = [], 0, 0
    for end in (int(e) for e in np.asarray(arrays["episode_ends"]).reshape(-1)):
        policy.reset()
        for t in range(first, end):
            img = arrays["img"][t:t + 1]
            if u8 and img.dtype != np.uint8:
                img = np.rint(img * 255).astype(np.uint8)                      # the store holds pixel / 255.0 (dataset.py)
            policy.observe(np.ascontiguousarray(img, dtype=np.uint8 if u8 else np.float32), arrays["position"][t:t + 1],
                           arrays["velocity"][t:t + 1], arrays["action"][t:t + 1])
            if (t - first) % args.replan_every:
                continue
            seed = args.seed + len(plans)
            x_T = torch.rand(K, 1, H, D, device=model.device, generator=torch.Generator(device=model.device).manual_seed(seed))
            torch.cuda.synchronize(model.device)
            start = time.perf_counter()
            if K > 1:
                plan = policy.plan_candidates(seed=seed, x_T=x_T, warm_start=args.warm_start, **many)
            elif args.warm_start is None:
                plan = policy.plan(seed=seed, x_T=x_T)
            else:
                plan = policy.plan(seed=seed, x_T=x_T, warm_start=args.warm_start)
            torch.cuda.synchronize(model.device)
            seconds = time.perf_counter() - start
            _, rows, out = plan_rows(t, first, end, obs_h, P, s)
            way = plan.waypoints[0, :len(rows)].cpu().numpy()
            d = position[rows] - way
            plans.append({"row": t, "episode_end": end, "errors": np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).tolist(),
                          "left_out": out, "seconds": seconds})
            if args.warm_start is not None:
                plans[-1].update(steps=plan.steps, warm=plan.warm)
            if K > 1:                                                          # after the clock has stopped
                j, how = int(plan.chosen[0].item()), policy.last_selection
                plans[-1].update(chosen=j, selected_by=plan.selected_by, scored_by=how["scored_by"], rows=how["rows"],
                                 score=float(plan.scores[0, j].item()), spread=plan.spread[0].cpu().tolist())
            left_out += out
        first = end
    def per_step(chosen):
        mean, std = [], []
        for j in range(P):
            col = np.array([p["errors"][j] for p in chosen if len(p["errors"]) > j], dtype=np.float64)
            mean.append(float(col.mean()) if col.size else None)
            std.append(float(col.std()) if col.size else None)
        return mean, std

    mean, std = per_step(plans)
    report = {"model_name": args.model_name, "obs_horizon": obs_h, "pred_horizon": P, "step_size": s, "replan_every": args.replan_every,
              "seed": args.seed, "image_storage": storage, "plans": plans, "left_out": left_out, "mean_error": mean, "std_error": std}
    if args.solver_steps is not None:
        report["solver"] = {"name": "dpmsolver++2m", "steps": args.solver_steps}
    if args.warm_start is not None:
        report["warm_start"] = args.warm_start
        for name, chosen in (("cold", [p for p in plans if not p["warm"]]), ("warm", [p for p in plans if p["warm"]])):
            report["mean_error_" + name], report["std_error_" + name] = per_step(chosen)
            report["seconds_" + name] = float(np.mean([p["seconds"] for p in chosen])) if chosen else None
        print(f"*** warm_start = {args.warm_start}: plan() mean {report['seconds_cold']} s cold, {report['seconds_warm']} s warm")
        print("mean position error per step, cold:", report["mean_error_cold"])
        print("mean position error per step, warm:", report["mean_error_warm"])
    if K > 1:
        report["candidates"], report["select"], report["select_cols"] = K, args.select, args.select_cols
        report["mean_spread"] = np.mean(np.array([p["spread"] for p in plans], dtype=np.float64), axis=0).tolist() if plans else None
        jumps = [p["score"] / (p["rows"] * args.select_cols) for p in plans if p["scored_by"] == "coherent"]
        report["mean_jump"] = float(np.mean(jumps)) if jumps else None
        print(f"*** candidates = {K}, select = {args.select}: mean squared step between consecutive plans {report['mean_jump']}")
        print("mean spread of the candidates per step:", report["mean_spread"])
    times = [p["seconds"] for p in plans]
    print(f"*** {len(plans)} plans, {left_out} way-points past an episode's end left out; plan(): median {np.median(times) * 1e3:.2f} ms")
    print("mean position error per step:", mean)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f)
    return report


if __name__ == "__main__":
    main()
