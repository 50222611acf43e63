"""evaluation.robustness on the GPU, on the small model and dataset of tests/test_gpu_eval.py: level 0 against evaluate(), a
noisy level against the host arm of tests/obs_noise_ref.py (the perturbation restated in numpy, the errors by tests/eval_ref.py).
Errors and per-window statistics are compared bit for bit; the means of squares are held to the bound of summation in any order."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import eval_ref
import obs_noise_ref
from test_gpu_eval import GOLDEN, M_OBS, M_PRED, SEED, T, U, _dataset, _model, same_bits

pytestmark = pytest.mark.gpu

IDS = [0, 90, 5, 90, 3]                                                              # 5 windows, one twice
RUNS = 2
LEVELS = (0.0, 0.05)
K, N = len(IDS), len(IDS) * RUNS


@functools.lru_cache(maxsize=None)
def _robust(batch_size):
    from state_policy_diffusionmodel_amd.evaluation import robustness
    return robustness(_model("DDPM"), _dataset(), IDS, levels=LEVELS, runs=RUNS, batch_size=batch_size, seed=SEED)


def test_level_zero_is_evaluate_bit_for_bit():
    from state_policy_diffusionmodel_amd.evaluation import EvalReport, evaluate
    rep = _robust(5)
    assert rep.levels.tolist() == list(LEVELS) and rep.draws.tolist() == [0, 1] and rep.window_ids.tolist() == IDS and rep.runs == RUNS
    assert rep.position_error.shape == (2, K, RUNS, M_PRED) and rep.action_error.shape == (2, K, RUNS, M_PRED, 3)
    assert rep.mean_error.shape == (2, M_PRED) and rep.action_window_std.shape == (2, K, M_PRED, 3)
    assert rep.mse_position.shape == rep.mse_action.shape == (2,)
    want = evaluate(_model("DDPM"), _dataset(), IDS, runs=RUNS, batch_size=5, seed=SEED)
    level0 = rep.level(0)
    for k in EvalReport.ARRAYS:
        same_bits(getattr(rep, k)[0], getattr(want, k), k)
        same_bits(getattr(level0, k), getattr(want, k), k + " of level(0)")
    assert not np.array_equal(rep.position_error[0], rep.position_error[1])          # the noise reached the sampler
    assert not np.array_equal(rep.action_error[0], rep.action_error[1])


@pytest.mark.parametrize("batch_size", [5, 64])
def test_a_noisy_level_equals_the_host_arm_bit_for_bit(batch_size):
    rep = _robust(batch_size)
    pos, act = obs_noise_ref.host_level(_model("DDPM"), _dataset(), IDS, runs=RUNS, batch_size=batch_size, seed=SEED, alpha=LEVELS[1], draw=1)
    assert np.isfinite(pos).all() and pos.max() > 0
    same_bits(rep.position_error[1].reshape(N, M_PRED), pos, "position_error")
    same_bits(rep.action_error[1].reshape(N, M_PRED, 3), act, "action_error")
    # one perturbation per (level, window): the two copies of window 90 sit in other rows and draw other noise
    assert not np.array_equal(rep.position_error[1, 1], rep.position_error[1, 3])
    for prefix, err in (("", pos), ("action_", act.reshape(N, -1))):
        wm, ws = eval_ref.window_stats(err, RUNS)
        same_bits(getattr(rep, prefix + "window_mean")[1].reshape(K, -1), wm, prefix + "window_mean")
        same_bits(getattr(rep, prefix + "window_std")[1].reshape(K, -1), ws, prefix + "window_std")
        mean, std = getattr(rep, prefix + "mean_error")[1].reshape(-1), getattr(rep, prefix + "std_error")[1].reshape(-1)
        for c in range(err.shape[1]):
            exact = math.fsum(err[:, c].tolist()) / N
            assert abs(mean[c] - exact) <= N * U * exact
            assert abs(std[c] - np.std(err[:, c])) <= 4 * N * U * (np.std(err[:, c]) + exact)


def test_a_level_alone_with_its_draw_equals_the_level_of_the_ladder():
    from state_policy_diffusionmodel_amd.evaluation import EvalReport, robustness
    rep = _robust(5)
    one = robustness(_model("DDPM"), _dataset(), IDS, levels=(0.05,), draws=(1,), runs=RUNS, batch_size=5, seed=SEED)
    assert one.position_error.shape == (1, K, RUNS, M_PRED)
    for k in EvalReport.ARRAYS:
        same_bits(getattr(one, k)[0], getattr(rep, k)[1], k)
    assert one.mse_position[0] == rep.mse_position[1] and one.mse_action[0] == rep.mse_action[1]
    other = robustness(_model("DDPM"), _dataset(), IDS, levels=(0.05,), draws=(2,), runs=RUNS, batch_size=5, seed=SEED)
    assert not np.array_equal(other.position_error[0], rep.position_error[1])        # another draw, another noise


def test_two_calls_give_identical_reports():
    from state_policy_diffusionmodel_amd.evaluation import EvalReport, robustness
    a = _robust(5)
    b = robustness(_model("DDPM"), _dataset(), IDS, levels=LEVELS, runs=RUNS, batch_size=5, seed=SEED)
    for k in EvalReport.ARRAYS:
        same_bits(getattr(a, k), getattr(b, k), k)
    assert np.array_equal(a.mse_position, b.mse_position) and np.array_equal(a.mse_action, b.mse_action)
    back = json.loads(a.to_json())
    assert back["levels"] == list(LEVELS) and np.array_equal(np.array(back["mse_action"]), a.mse_action)
    assert np.array_equal(np.array(back["position_error"]), a.position_error)


def test_the_report_does_not_depend_on_the_batch_size():
    """The observation noise is keyed by the window's place in the list, not by the chunk, so batch sizes differ only through the
    sampler's choice of kernels: the 1e-4 trajectory tolerance of test_gpu_eval.py, pushed through the unnormalisation."""
    a, b = _robust(5), _robust(64)
    st = _dataset().stats["position"]
    bound = math.sqrt(2.0) * 1e-4 * (float(st["max"]) - float(st["min"]))
    for lev in range(len(LEVELS)):
        diff = float(np.abs(a.position_error[lev] - b.position_error[lev]).max())
        print(f"level {lev}: max |position_error(batch_size 5) - position_error(batch_size 64)| = {diff:.3e}, bound {bound:.3e}")
        assert diff <= bound


def test_the_mean_squared_errors_equal_numpy_within_the_summation_bound():
    rep = _robust(5)
    for lev in range(len(LEVELS)):
        want_pos = float(np.mean(np.square(rep.position_error[lev]))) / 2             # over both coordinates
        want_act = float(np.mean(np.square(rep.action_error[lev])))
        n_pos, n_act = rep.position_error[lev].size, rep.action_error[lev].size
        print(f"level {lev}: mse_position {rep.mse_position[lev]:.6e} (numpy {want_pos:.6e}, bound {n_pos * U * want_pos:.1e}), "
              f"mse_action {rep.mse_action[lev]:.6e} (numpy {want_act:.6e}, bound {n_act * U * want_act:.1e})")
        assert want_pos > 0 and want_act > 0
        assert abs(rep.mse_position[lev] - want_pos) <= n_pos * U * want_pos
        assert abs(rep.mse_action[lev] - want_act) <= n_act * U * want_act


def test_the_command_line_writes_the_same_numbers(tmp_path):
    """python -m state_policy_diffusionmodel_amd.evaluate --noise_levels on files written here (in process: the test starts
    nothing) against robustness() on the same model and data; without the flag the JSON has no "robustness"."""
    import yaml
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd import weights
    from state_policy_diffusionmodel_amd.dataset import CarRacingDataModule
    from state_policy_diffusionmodel_amd.evaluate import main
    from state_policy_diffusionmodel_amd.evaluation import EvalReport, robustness
    hp = dict(noise_steps=6, obs_horizon=M_OBS, pred_horizon=M_PRED, observation_dim=135, prediction_dim=5, learning_rate=1e-4,
              model="UNet_FilmnoAttention", noise_scheduler_type="linear", inpaint_horizon=1, step_size=1)
    sd = weights.random_state_dict(135 * M_OBS, seed=3, attention=False, model="UNet_FilmnoAttention", noise_steps=6)
    full = {"noise_estimator." + k: torch.from_numpy(np.array(v)) for k, v in weights.state_dict_to_numpy(sd).items()}
    full.update({"vision_encoder." + k: v for k, v in make_encoder_state_dict(7).items()})
    paths = {k: str(tmp_path / k) for k in ("epoch=0.ckpt", "hparams.yaml", "STATS.pkl", "arrays.npz", "report.json", "plain.json")}
    torch.save({"state_dict": full}, paths["epoch=0.ckpt"])
    with open(paths["hparams.yaml"], "w") as f:
        f.write(yaml.safe_dump(hp))
    dm = CarRacingDataModule(1)
    dm.stats = _dataset().stats
    dm.save_stats(paths["STATS.pkl"])
    g = np.load(GOLDEN)
    np.savez(paths["arrays.npz"], position=g["position"], velocity=g["velocity"], action=g["action"], episode_ends=g["episode_ends"],
             img=np.random.default_rng(5).integers(0, 256, (T, 96, 96, 3), dtype=np.uint8))
    common = ["--model_name", "DDPM", "--checkpoint", paths["epoch=0.ckpt"], "--hparams", paths["hparams.yaml"], "--stats", paths["STATS.pkl"],
              "--data", paths["arrays.npz"], "--runs", "1", "--batch_size", "64", "--seed", str(SEED)]
    main(common + ["--noise_levels", "0,0.05", "--out", paths["report.json"]])
    want = robustness(_model("DDPM"), _dataset(), None, levels=LEVELS, runs=1, batch_size=64, seed=SEED)
    back = json.load(open(paths["report.json"]))
    rob = back["robustness"]
    assert rob["levels"] == list(LEVELS) and rob["draws"] == [0, 1] and rob["window_ids"] == list(range(91))
    for k in EvalReport.ARRAYS + ("mse_position", "mse_action"):
        same_bits(np.array(rob[k], dtype=np.float64), getattr(want, k), k)
    same_bits(np.array(back["position_error"]), want.position_error[0], "the plain report beside it")
    main(common + ["--out", paths["plain.json"]])
    plain = json.load(open(paths["plain.json"]))
    assert "robustness" not in plain and plain == {k: v for k, v in back.items() if k != "robustness"}
