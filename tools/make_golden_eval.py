#!/usr/bin/env python3
"""Record the evaluation fixture tests/golden/eval_small.npz.

    python tools/make_golden_eval.py <path to a checkout of the reference project>

Runs only where the reference exists.  It calls the reference's OWN utils/data_utils.py functions (unnormalize_position,
unnormalize_data) the way evaluation/eval_acurracy_diffusion_positions.py:118-140 does, one trajectory at a time, on the
windows, translations and statistics of tests/golden/dataset_small.npz (truth rounded to float32, as the model's batch holds
it) and on seeded float32 predictions, and stores only data: per case the window numbers, the predictions, the per-element
position and action errors, and np.mean / np.std of them over all rows and per window.  The action error is this project's
metric; the reference contributes its unnormalize_data.  tests/test_eval_reference.py reads it.
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np

SRC = os.path.join(ROOT, "tests", "golden", "dataset_small.npz")
OUT = os.path.join(ROOT, "tests", "golden", "eval_small.npz")
SEQ, OBS, P = 6, 2, 4
# (dataset key, windows, runs, inpaint horizon, D)
CASES = [("s5", list(range(58)), 3, 1, 5),
         ("s1", list(range(20)), 1, 0, 2),
         ("s1", list(range(100, 124)), 3, 2, 5),
         ("s5", [57, 0, 31, 31, 8, 40, 2, 19, 50, 11], 1, 2, 2),
         ("s1", [0, 123, 60, 61, 62, 5, 5, 99, 17, 80], 3, 0, 5),
         ("s5", [3, 9, 27, 44, 56, 12, 1, 33, 20, 48], 1, 1, 5)]


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "utils")):
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from utils import data_utils as du

    g = np.load(SRC)
    rng = np.random.default_rng(20241019)
    out = {"n_cases": len(CASES), "seq": SEQ, "obs_h": OBS, "P": P}
    for i, (key, windows, runs, inp, D) in enumerate(CASES):
        pos_stats = {"min": g[key + "/pos_min"][()], "max": g[key + "/pos_max"][()]}
        act_stats = {"min": g[key + "/act_min"], "max": g[key + "/act_max"]}
        truth_pos = g[key + "/position"].astype(np.float32)         # (N, SEQ, 2): the model's batch is float32
        truth_act = g[key + "/action"].astype(np.float32)
        translation = g[key + "/translation"]
        B = len(windows) * runs
        # predictions near the truth (as a trained model's are) plus the odd far one
        pred = rng.uniform(-1.0, 1.0, (B, inp + P, D)).astype(np.float32)
        for b in range(0, B, 2):
            k = windows[b // runs]
            near = np.concatenate([truth_pos[k, OBS - inp:], truth_act[k, OBS - inp:]], axis=1)[:, :D]
            pred[b] = near + (0.05 * rng.standard_normal(near.shape)).astype(np.float32)
        pos_err, act_err = [], []
        for b in range(B):
            k = windows[b // runs]
            gt = du.unnormalize_position(truth_pos[k][None], translation[k], pos_stats)
            pr = du.unnormalize_position(pred[b, :, 0:2], translation[k], pos_stats)
            pos_err.append(np.linalg.norm(gt[0, OBS:, :] - pr[inp:], axis=1))
            if D >= 5:
                act_err.append(np.abs(du.unnormalize_data(truth_act[k, OBS:], act_stats) -
                                      du.unnormalize_data(pred[b, inp:, 2:5], act_stats)))
        c = f"c{i}/"
        out.update({c + "key": key, c + "windows": np.array(windows, np.int64), c + "runs": runs, c + "inp_h": inp, c + "D": D,
                    c + "pred": pred})
        for name, err in (("pos", np.array(pos_err)),) + ((("act", np.array(act_err)),) if D >= 5 else ()):
            assert err.dtype == np.float64
            out[c + name + "_err"] = err
            out[c + name + "_mean"] = np.mean(err, axis=0)
            out[c + name + "_std"] = np.std(err, axis=0)
            per = err.reshape((len(windows), runs) + err.shape[1:])
            out[c + name + "_window_mean"] = np.array([np.mean(w, axis=0) for w in per])
            out[c + name + "_window_std"] = np.array([np.std(w, axis=0) for w in per])
        print(f"case {i}: {key}, {len(windows)} windows x {runs} runs, inp {inp}, D {D}: mean position error "
              f"{np.mean(pos_err):.4f}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
