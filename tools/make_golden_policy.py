#!/usr/bin/env python3
"""Record the closed-loop policy fixture tests/golden/policy_small.npz.

    python tools/make_golden_policy.py <path to a checkout of the reference project>

Runs only where the reference exists.  It drives the reference's OWN utils/data_utils.py functions (normalize_data,
normalize_position, unnormalize_position) exactly as run_predictions.py does: four deque(maxlen = obs_horizon * step_size), the
initial fill of :120-124 (which is also what a reset is), one append per step, and prepare_diffusion_batch's
list(deque)[::s] -> torch.tensor(..., dtype=torch.float32) -> normalize (:30-60), followed by the model's .float().  The
observation stream is the positions, velocities and actions of tests/golden/dataset_small.npz, row by row; the statistics are
that fixture's, once as float64 arrays and once as float32 arrays (torch promotes by the arrays' dtype).  Only data is stored:
per case and per push the low-dimensional batch, and one block of unnormalize_position results on float32 inputs.  Frames are
not recorded: float32(k) / 255 is pinned by tests/test_dataset_reference.py.  tests/test_policy_reference.py reads it.
"""
import os
import sys
from collections import deque

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

SRC = os.path.join(ROOT, "tests", "golden", "dataset_small.npz")
OUT = os.path.join(ROOT, "tests", "golden", "policy_small.npz")
# (obs_horizon, step_size, first row, pushes, pushes that are preceded by a reset, statistics dtype)
CASES = [(1, 1, 0, 3, [0], "float64"),
         (2, 3, 0, 11, [0], "float64"),                  # wraps L = 6
         (2, 3, 5, 11, [0], "float32"),
         (4, 5, 61, 47, [0, 23], "float64"),             # wraps L = 20 twice, with a reset mid-stream
         (4, 5, 61, 47, [0, 23], "float32"),
         (10, 5, 0, 60, [0], "float64")]                 # the reference's defaults: L = 50


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "utils")):
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from utils import data_utils as du

    g = np.load(SRC)
    out = {"n_cases": len(CASES), "numpy": np.__version__, "torch": torch.__version__}
    last_translation = []
    for i, (obs_h, s, first, pushes, resets, dt) in enumerate(CASES):
        L = obs_h * s
        stats = {"position": {"min": g["s5/pos_min"][()], "max": g["s5/pos_max"][()]},
                 "velocity": {k: g["s5/vel_" + k].astype(dt) for k in ("min", "max")},
                 "action": {k: g["s5/act_" + k].astype(dt) for k in ("min", "max")}}
        assert isinstance(stats["position"]["min"], np.float64)
        bufs = {k: deque(maxlen=L) for k in ("position", "velocity", "action")}
        rec = {k: [] for k in ("position", "velocity", "action", "translation")}
        for n in range(pushes):
            obs = {k: g[k][first + n] for k in bufs}
            for k in bufs:
                if n in resets:
                    for _ in range(L):                     # run_predictions.py:120-124
                        bufs[k].append(obs[k])
                else:
                    bufs[k].append(obs[k])                 # :145-148
            batch = {k: torch.tensor(list(list(bufs[k])[::s]), dtype=torch.float32) for k in bufs}       # :33-44
            na = du.normalize_data(batch["action"], stats["action"])
            nv = du.normalize_data(batch["velocity"], stats["velocity"])
            npos, tr = du.normalize_position(batch["position"], stats["position"])
            assert na.dtype == nv.dtype == getattr(torch, dt) and npos.dtype == tr.dtype == torch.float32
            for k, v in (("position", npos), ("velocity", nv), ("action", na), ("translation", tr)):
                rec[k].append(v.float().numpy().copy())    # models/diffusion_ddpm.py:287-290
        c = f"c{i}/"
        out.update({c + "obs_h": obs_h, c + "step_size": s, c + "first": first, c + "pushes": pushes,
                    c + "resets": np.array(resets, np.int64), c + "stats_dtype": dt})
        out.update({c + k: np.stack(v) for k, v in rec.items()})
        last_translation.append(rec["translation"][-1])
        print(f"case {i}: obs_h {obs_h}, step {s}, {pushes} pushes from row {first}, resets {resets}, {dt} statistics")
    # unnormalize_position as run_predictions.py:159-164 calls it: float32 numpy prediction and translation
    rng = np.random.default_rng(20241020)
    pred = rng.uniform(-1.0, 1.0, (len(CASES), 16, 2)).astype(np.float32)
    pos_stats = {"min": g["s5/pos_min"][()], "max": g["s5/pos_max"][()]}
    un = np.stack([du.unnormalize_position(pred[i], last_translation[i], pos_stats) for i in range(len(CASES))])
    out.update({"un/pred": pred, "un/translation": np.stack(last_translation), "un/out": un})
    print("unnormalize_position returns", un.dtype)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
