"""The evaluation metric on the GPU (evaluation.py, csrc/evaluation.hip: spdm_eval_errors, spdm_eval_reduce) against
tests/eval_ref.py.  Errors and per-window statistics are chains of correctly rounded float64 (and two float32) operations in a
fixed order, so their tolerance is zero; the all-rows statistics are held to the bounds of summation in any order."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import eval_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_small.npz")
OBS = 2
STATS = {"position": {"min": np.float64(-37.3), "max": np.float64(52.9)},
         "action": {"min": np.array([-1.0, 0.0, 0.0]), "max": np.array([1.0, 0.95, 0.8])}}
U = 2.0 ** -53


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, got.dtype, want.shape, want.dtype)
    diff = np.count_nonzero(got.view(np.uint64) != want.view(np.uint64))
    assert diff == 0, f"{what}: {diff} of {got.size} elements differ"


# ---- spdm_eval_errors -------------------------------------------------------------------------------------------------------
def _errors_case(B, runs, P, inp, D, first_traj=0, window_base=0, spare_slots=0):
    from state_policy_diffusionmodel_amd.evaluation import errors_into
    rng = np.random.default_rng([B, runs, P, inp, D, first_traj])
    slot = eval_ref.slots(first_traj, B, runs, window_base)
    n_slots, seq = int(slot[-1]) + 1 + spare_slots, OBS + P + 1                      # one truth row more than is read
    tp = rng.uniform(-1, 1, (n_slots, seq, 2)).astype(np.float32)
    ta = rng.uniform(-1, 1, (n_slots, seq, 3)).astype(np.float32)
    tr = rng.uniform(-1, 1, (n_slots, 2))
    pred = rng.uniform(-1.2, 1.2, (B, inp + P, D)).astype(np.float32)
    pred[::2, inp:, 0:2] = tp[slot[::2], OBS:OBS + P] + (1e-3 * rng.standard_normal((len(slot[::2]), P, 2))).astype(np.float32)
    actions = D >= 5
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    batch = {"position": dev(tp), "action": dev(ta), "translation": dev(tr)}
    pos = torch.full((B, P), -1.0, dtype=torch.float64, device="cuda")
    act = torch.full((B, P, 3), -1.0, dtype=torch.float64, device="cuda") if actions else None
    errors_into(dev(pred).view(B, 1, inp + P, D), batch, STATS, obs_h=OBS, inp_h=inp, runs=runs, first_traj=first_traj,
                window_base=window_base, pos_err=pos, act_err=act)
    what = dict(B=B, runs=runs, P=P, inp=inp, D=D, first_traj=first_traj)
    want = eval_ref.position_errors(pred, tp, tr, slot, STATS["position"]["min"], STATS["position"]["max"], OBS, inp, P)
    assert np.isfinite(want).all() and want.max() > 0
    same_bits(pos.cpu().numpy(), want, ("position", what))
    if actions:
        same_bits(act.cpu().numpy(), eval_ref.action_errors(pred, ta, slot, STATS["action"]["min"], STATS["action"]["max"], OBS, inp, P),
                  ("action", what))


@pytest.mark.parametrize("runs", [1, 3])
@pytest.mark.parametrize("B", [1, 7, 300])
def test_errors_equal_the_restatement_bit_for_bit(B, runs):
    for P in (1, 4):
        for inp in (0, 1, 2):
            for D in (2, 5):                                                         # D = 2: no action output
                _errors_case(B, runs, P, inp, D)


def test_a_chunk_that_begins_inside_a_window_with_a_window_base():
    _errors_case(40, 3, 4, 1, 5, first_traj=3 * 7 + 2, window_base=5, spare_slots=2)    # rows 23 .. 62: slots 2 .. 15 of 18
    _errors_case(300, 3, 4, 2, 5, first_traj=3 * 1000 + 1, window_base=1000)           # more than one workgroup
    _errors_case(5, 7, 1, 0, 2, first_traj=7 * 3 + 2, window_base=3)                    # all rows inside ONE window's runs


def test_errors_on_the_recorded_fixture():
    """The kernel against what the reference's own functions gave (tests/golden/eval_small.npz, case 0)."""
    from state_policy_diffusionmodel_amd.evaluation import errors_into
    g, d = np.load(os.path.join(os.path.dirname(GOLDEN), "eval_small.npz")), np.load(GOLDEN)
    w, pred = g["c0/windows"], g["c0/pred"]
    stats = {"position": {"min": d["s5/pos_min"], "max": d["s5/pos_max"]}, "action": {"min": d["s5/act_min"], "max": d["s5/act_max"]}}
    batch = {"position": torch.from_numpy(d["s5/position"].astype(np.float32)[w]).cuda(),
             "action": torch.from_numpy(d["s5/action"].astype(np.float32)[w]).cuda(),
             "translation": torch.from_numpy(d["s5/translation"][w]).cuda()}
    B = len(pred)
    pos = torch.empty((B, 4), dtype=torch.float64, device="cuda")
    act = torch.empty((B, 4, 3), dtype=torch.float64, device="cuda")
    errors_into(torch.from_numpy(pred).cuda(), batch, stats, obs_h=2, inp_h=1, runs=3, first_traj=0, window_base=0, pos_err=pos, act_err=act)
    same_bits(pos.cpu().numpy(), g["c0/pos_err"], "position")
    same_bits(act.cpu().numpy(), g["c0/act_err"], "action")


# ---- spdm_eval_reduce -------------------------------------------------------------------------------------------------------
# N = 3000 is three blocks of rows, the last one partial (a block is 1024 rows); the others are the single-block sizes
@pytest.mark.parametrize("C", [1, 7, 12])
@pytest.mark.parametrize("N,runs", [(1, 1), (21, 3), (21, 1), (1000, 1), (1000, 8), (3000, 3)])
def test_reduce(N, runs, C):
    from state_policy_diffusionmodel_amd.evaluation import reduce_errors
    rng = np.random.default_rng([N, runs, C])
    err = np.abs(rng.standard_normal((N, C)) * 30.0) + rng.uniform(0, 5, (1, C))    # non-negative, as errors are
    d_err = torch.from_numpy(err).cuda()
    got = [t.cpu().numpy() for t in reduce_errors(d_err, runs)]
    again = [t.cpu().numpy() for t in reduce_errors(d_err, runs)]
    for a, b, name in zip(got, again, ("window_mean", "window_std", "mean", "std")):
        same_bits(a, b, name + " of a second call")
    wmean, wstd, mean, std = got
    want_mean, want_std = eval_ref.window_stats(err, runs)
    same_bits(wmean, want_mean, "window mean")
    same_bits(wstd, want_std, "window std")
    if runs == 1:
        assert not wstd.any() and np.array_equal(wmean, err)
    if N == 1:
        assert not std.any() and np.array_equal(mean, err[0])
    np_std = np.std(err, axis=0)
    for c in range(C):
        exact = math.fsum(err[:, c].tolist()) / N
        rel = abs(mean[c] - exact) / exact
        print(f"N {N} C {C} column {c}: mean rel err {rel:.3e} (bound {N * U:.3e}), std diff {abs(std[c] - np_std[c]):.3e} "
              f"(bound {4 * N * U * (np_std[c] + exact):.3e})")
        assert rel <= N * U, (c, rel)
        assert abs(std[c] - np_std[c]) <= 4 * N * U * (np_std[c] + exact), (c, std[c], np_std[c])


# ---- end to end -------------------------------------------------------------------------------------------------------------
T, M_OBS, M_PRED, RUNS, SEED = 140, 2, 15, 3, 11
IDS = [0, 90, 5, 90, 3, 44, 17]                                                      # 7 windows, one twice


@functools.lru_cache(maxsize=None)
def _dataset():
    from state_policy_diffusionmodel_amd.dataset import DeviceDataset
    g = np.load(GOLDEN)
    img = np.random.default_rng(5).integers(0, 256, (T, 96, 96, 3), dtype=np.uint8)
    d = DeviceDataset(g["position"], g["velocity"], g["action"], img, g["episode_ends"], M_PRED, M_OBS, step_size=1)
    assert len(d) == 91
    return d


@functools.lru_cache(maxsize=None)
def _model(kind):
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd.diffusion import load_model
    return load_model(kind, None, None, num_of_ddim_steps=6, model="UNet_FilmnoAttention", noise_steps=6, obs_horizon=M_OBS,
                      pred_horizon=M_PRED, inpaint_horizon=1, observation_dim=135, prediction_dim=5,
                      vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=64, weight_seed=3)


@functools.lru_cache(maxsize=None)
def _report(kind, batch_size):
    from state_policy_diffusionmodel_amd.evaluation import evaluate
    return evaluate(_model(kind), _dataset(), IDS, runs=RUNS, batch_size=batch_size, seed=SEED)


def _host_way(kind, batch_size):
    """The same chunks the host way: sample, fetch x_0, eval_ref.  The chunking is restated here, not imported."""
    from state_policy_diffusionmodel_amd.evaluation import initial_noise
    model, d = _model(kind), _dataset()
    N = len(IDS) * RUNS
    x_T = initial_noise(model, N, SEED)
    st = d.stats
    pos, act = [], []
    for g0 in range(0, N, batch_size):
        g1 = min(N, g0 + batch_size)
        k0, k1 = g0 // RUNS, (g1 - 1) // RUNS + 1
        batch = d.batch(IDS[k0:k1], frames="obs", with_translation=True)
        obs = model.prepare_observation_batch(batch)
        cond, inpaint = model.prepare_obs_cond_vectors(obs), model.prepare_inpaint_vectors(obs)
        slot = eval_ref.slots(g0, g1 - g0, RUNS, k0)
        sel = torch.from_numpy(slot).cuda()
        x_0 = model.sample({"obs_cond": cond[sel], "inpaint": inpaint[sel]}, batched=True, sharded=False, x_T=x_T[g0:g1], seed=SEED,
                           sample_offset=g0)
        x_0 = x_0.cpu().numpy()[:, 0]
        tp, ta, tr = (batch[k].cpu().numpy() for k in ("position", "action", "translation"))
        pos.append(eval_ref.position_errors(x_0, tp, tr, slot, float(st["position"]["min"]), float(st["position"]["max"]), M_OBS, 1, M_PRED))
        act.append(eval_ref.action_errors(x_0, ta, slot, st["action"]["min"], st["action"]["max"], M_OBS, 1, M_PRED))
    return np.concatenate(pos), np.concatenate(act)


@pytest.mark.parametrize("kind,batch_size", [("DDPM", 5), ("DDPM", 64), ("DDIM", 5)])
def test_evaluate_equals_the_host_way_bit_for_bit(kind, batch_size):
    rep = _report(kind, batch_size)
    K, N = len(IDS), len(IDS) * RUNS
    assert rep.position_error.shape == (K, RUNS, M_PRED) and rep.action_error.shape == (K, RUNS, M_PRED, 3)
    assert rep.mean_error.shape == rep.std_error.shape == (M_PRED,) and rep.window_mean.shape == rep.window_std.shape == (K, M_PRED)
    assert rep.action_mean_error.shape == (M_PRED, 3) and rep.action_window_std.shape == (K, M_PRED, 3)
    assert np.isfinite(rep.position_error).all() and rep.position_error.max() > 0
    pos, act = _host_way(kind, batch_size)
    same_bits(rep.position_error.reshape(N, M_PRED), pos, "position_error")
    same_bits(rep.action_error.reshape(N, M_PRED, 3), act, "action_error")
    # runs of one window differ (their noise is keyed by the trajectory), the two copies of window 90 are different trajectories
    assert not np.array_equal(rep.position_error[0, 0], rep.position_error[0, 1])
    assert not np.array_equal(rep.position_error[1], rep.position_error[3])
    for prefix, err in (("", pos), ("action_", act.reshape(N, -1))):
        wm, ws = eval_ref.window_stats(err, RUNS)
        same_bits(getattr(rep, prefix + "window_mean").reshape(K, -1), wm, prefix + "window_mean")
        same_bits(getattr(rep, prefix + "window_std").reshape(K, -1), ws, prefix + "window_std")
        mean, std = getattr(rep, prefix + "mean_error").reshape(-1), getattr(rep, prefix + "std_error").reshape(-1)
        for c in range(err.shape[1]):
            exact = math.fsum(err[:, c].tolist()) / N
            assert abs(mean[c] - exact) <= N * U * exact
            assert abs(std[c] - np.std(err[:, c])) <= 4 * N * U * (np.std(err[:, c]) + exact)
    back = json.loads(rep.to_json())
    assert back["window_ids"] == IDS and back["runs"] == RUNS and np.array_equal(np.array(back["mean_error"]), rep.mean_error)


def test_the_report_does_not_depend_on_the_batch_size():
    a, b = _report("DDPM", 5), _report("DDPM", 64)
    st = _dataset().stats["position"]
    bound = math.sqrt(2.0) * 1e-4 * (float(st["max"]) - float(st["min"]))
    diff = float(np.abs(a.position_error - b.position_error).max())
    print(f"max |position_error(batch_size 5) - position_error(batch_size 64)| = {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound


def test_two_evaluations_give_identical_reports():
    from state_policy_diffusionmodel_amd.evaluation import EvalReport, evaluate
    a = _report("DDPM", 5)
    b = evaluate(_model("DDPM"), _dataset(), IDS, runs=RUNS, batch_size=5, seed=SEED)
    for k in EvalReport.ARRAYS:
        same_bits(getattr(a, k), getattr(b, k), k)
    c = evaluate(_model("DDPM"), _dataset(), IDS[:2], runs=2, batch_size=64, seed=SEED + 1, actions=False)
    assert c.action_error is None and c.position_error.shape == (2, 2, M_PRED)
    assert not np.array_equal(c.position_error[0, 0], a.position_error[0, 0])       # another seed


def test_evaluate_refuses_what_it_cannot_measure():
    from state_policy_diffusionmodel_amd.dataset import DeviceDataset
    from state_policy_diffusionmodel_amd.evaluation import evaluate
    with pytest.raises(IndexError):
        evaluate(_model("DDPM"), _dataset(), [0, 91])
    with pytest.raises(ValueError):
        evaluate(_model("DDPM"), _dataset(), [0], runs=0)
    g = np.load(GOLDEN)
    other = DeviceDataset(g["position"], g["velocity"], g["action"], np.zeros((T, 96, 96, 3), np.uint8), g["episode_ends"], 4, M_OBS)
    with pytest.raises(ValueError, match="pred"):
        evaluate(_model("DDPM"), other, [0])


def test_the_command_line_gives_the_same_report(tmp_path):
    """python -m state_policy_diffusionmodel_amd.evaluate on a checkpoint, hparams.yaml, STATS.pkl and arrays.npz written here
    (in process: the test starts nothing) against evaluate() on the same model and data."""
    import yaml
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd import weights
    from state_policy_diffusionmodel_amd.dataset import CarRacingDataModule
    from state_policy_diffusionmodel_amd.evaluate import main
    from state_policy_diffusionmodel_amd.evaluation import EvalReport, evaluate
    hp = dict(noise_steps=6, obs_horizon=M_OBS, pred_horizon=M_PRED, observation_dim=135, prediction_dim=5, learning_rate=1e-4,
              model="UNet_FilmnoAttention", noise_scheduler_type="linear", inpaint_horizon=1, step_size=1)
    sd = weights.random_state_dict(135 * M_OBS, seed=3, attention=False, model="UNet_FilmnoAttention", noise_steps=6)
    full = {"noise_estimator." + k: torch.from_numpy(np.array(v)) for k, v in weights.state_dict_to_numpy(sd).items()}
    full.update({"vision_encoder." + k: v for k, v in make_encoder_state_dict(7).items()})
    paths = {k: str(tmp_path / k) for k in ("epoch=0.ckpt", "hparams.yaml", "STATS.pkl", "arrays.npz", "report.json")}
    torch.save({"state_dict": full}, paths["epoch=0.ckpt"])
    with open(paths["hparams.yaml"], "w") as f:
        f.write(yaml.safe_dump(hp))
    dm = CarRacingDataModule(1)
    dm.stats = _dataset().stats
    dm.save_stats(paths["STATS.pkl"])
    g = np.load(GOLDEN)
    np.savez(paths["arrays.npz"], position=g["position"], velocity=g["velocity"], action=g["action"], episode_ends=g["episode_ends"],
             img=np.random.default_rng(5).integers(0, 256, (T, 96, 96, 3), dtype=np.uint8))
    got = main(["--model_name", "DDPM", "--checkpoint", paths["epoch=0.ckpt"], "--hparams", paths["hparams.yaml"], "--stats", paths["STATS.pkl"],
                "--data", paths["arrays.npz"], "--runs", "1", "--batch_size", "64", "--seed", str(SEED), "--out", paths["report.json"]])
    want = evaluate(_model("DDPM"), _dataset(), None, runs=1, batch_size=64, seed=SEED)
    assert got.position_error.shape == (91, 1, M_PRED)
    for k in EvalReport.ARRAYS:
        same_bits(getattr(got, k), getattr(want, k), k)
    back = json.load(open(paths["report.json"]))
    assert np.array_equal(np.array(back["std_error"]), want.std_error) and back["window_ids"] == list(range(91))
