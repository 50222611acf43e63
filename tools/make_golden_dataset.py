#!/usr/bin/env python3
"""Record the dataset fixture tests/golden/dataset_small.npz.

    python tools/make_golden_dataset.py <path to a checkout of the reference project>

Runs only where the reference exists.  It calls the reference's OWN utils/data_utils.py functions
(create_sample_indices_sparse, sample_sequence_array_sparse, get_data_stats, normalize_data, normalize_position) in the order
CarRacingDataset uses them (utils/load_data.py:28-99) on small seeded float64 arrays and stores only data: the inputs, both
index tables (step_size 5 and 1), the statistics, the whole-array normalised velocity and action, and for every window the
sampled-and-normalised position, its translation, and the sampled velocity and action.  Images are not recorded: their
transform (moveaxis + a division by 255) is checked against numpy inside the tests.  tests/test_dataset_reference.py reads it.
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np

OUT = os.path.join(ROOT, "tests", "golden", "dataset_small.npz")
T, ENDS, SEQ, STEPS = 140, [37, 60, 61, 140], 6, (5, 1)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "utils")):
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from utils import data_utils as du

    rng = np.random.default_rng(20240607)
    position = 30.0 * rng.standard_normal((T, 2))
    velocity = 12.0 * rng.standard_normal((T, 2))
    action = rng.uniform(-1.0, 1.0, (T, 3))
    out = {"position": position, "velocity": velocity, "action": action, "episode_ends": np.array(ENDS, np.int64),
           "sequence_length": SEQ}
    for step in STEPS:
        indices = np.array(du.create_sample_indices_sparse(ENDS, SEQ, step), dtype=np.int64)
        pmin, pmax = [], []
        for start, end, _, _ in indices:              # _compute_stats
            st = du.get_data_stats(du.sample_sequence_array_sparse(position, step, start, end))
            pmax.append(st["max"])
            pmin.append(st["min"])
        pos_stats = {"max": np.average(pmax), "min": np.average(pmin)}
        vel_stats, act_stats = du.get_data_stats(velocity), du.get_data_stats(action)
        nvel, nact = du.normalize_data(velocity, vel_stats), du.normalize_data(action, act_stats)
        data = {"position": position, "velocity": nvel, "action": nact}
        pos, trans, vel, act = [], [], [], []
        for start, end, _, _ in indices:              # __getitem__, inference flavour (it also returns the translation)
            s = du.sample_sequence_sparse(data, step, start, end)
            p, tr = du.normalize_position(s["position"], pos_stats)
            pos.append(p)
            trans.append(tr)
            vel.append(s["velocity"])
            act.append(s["action"])
        k = f"s{step}/"
        out.update({k + "indices": indices, k + "pos_min": pos_stats["min"], k + "pos_max": pos_stats["max"],
                    k + "vel_min": vel_stats["min"], k + "vel_max": vel_stats["max"], k + "act_min": act_stats["min"],
                    k + "act_max": act_stats["max"], k + "position": np.array(pos), k + "translation": np.array(trans),
                    k + "velocity": np.array(vel), k + "action": np.array(act)})
        print(f"step_size {step}: {len(indices)} windows, last ends at row {indices[-1, 1]}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
