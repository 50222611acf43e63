"""The closed-loop policy on the GPU (policy.py, csrc/policy.hip: spdm_policy_push, spdm_policy_window, spdm_policy_unnormalize)
against tests/policy_ref.py, bit for bit: every operation involved is an exact copy or a correctly rounded float32 / float64
operation in a fixed order, so the tolerance is zero."""
import functools
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch

import policy_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_small.npz")


@functools.lru_cache(maxsize=None)
def _stats(dt):
    d = np.load(GOLDEN)
    return {"position": {"min": d["s5/pos_min"][()], "max": d["s5/pos_max"][()]},
            "velocity": {k: d["s5/vel_" + k].astype(dt) for k in ("min", "max")},
            "action": {k: d["s5/act_" + k].astype(dt) for k in ("min", "max")}}


def _geometry(obs_h, step_size, pred=1, inp=0, D=5):
    """What ClosedLoopPolicy reads of a model, for the tests that sample nothing."""
    return types.SimpleNamespace(obs_horizon=obs_h, pred_horizon=pred, inpaint_horizon=inp, prediction_dim=D, step_size=step_size,
                                 device=torch.device("cuda", 0))


def _same_bits(got: torch.Tensor, want: np.ndarray, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = np.count_nonzero(np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits))
    assert diff == 0, f"{what}: {diff} of {got.size} elements differ"


def _observations(E, pushes, storage, seed):
    """Per push: frames (seeded integers(0, 256); as float32 values k / 255 for float32 storage) and float64 low-dimensional
    values, which the policy rounds to float32 on entry."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(pushes):
        img = rng.integers(0, 256, (E, 96, 96, 3), dtype=np.uint8)
        if storage == "float32":
            img = (img / 255.0).astype(np.float32)
        out.append((img, 30.0 * rng.standard_normal((E, 2)), 12.0 * rng.standard_normal((E, 2)), rng.uniform(-1.0, 1.0, (E, 3))))
    return out


# ---- spdm_policy_push, spdm_policy_window ------------------------------------------------------------------------------------
@pytest.mark.parametrize("stats_dtype", ["float64", "float32"])
@pytest.mark.parametrize("storage", ["uint8", "float32"])
@pytest.mark.parametrize("E,obs_h,step_size,pushes,reset_after", [(1, 1, 1, 1, None), (3, 2, 3, 11, None), (5, 4, 5, 47, 23)])
def test_push_and_window_equal_the_restatement_bit_for_bit(E, obs_h, step_size, pushes, reset_after, storage, stats_dtype):
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    stats = _stats(stats_dtype)
    L = obs_h * step_size
    policy = ClosedLoopPolicy(_geometry(obs_h, step_size), stats, n_envs=E, image_storage=storage)
    ref = policy_ref.History(E, L)
    # compared after these many pushes: the first two, around each wrap of the ring, around the reset, and the last
    look = {1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1, pushes} | ({reset_after + 1, reset_after + 2, reset_after + 3} if reset_after else set())
    for n, (img, pos, vel, act) in enumerate(_observations(E, pushes, storage, [E, obs_h, step_size])):
        if n % 2:                                                               # device inputs on odd pushes, host inputs on even
            policy.observe(*(torch.from_numpy(x).cuda() for x in (img, pos, vel, act)))
        else:
            policy.observe(img, pos, vel, act)
        ref.push(img, pos, vel, act)
        if n == reset_after:                                                    # push number 23 is done: the next one refills 1 and 3
            policy.reset([1, 3])
            ref.reset([1, 3])
        if n + 1 in look:
            got, want = policy.batch(), policy_ref.batch(ref, stats, step_size)
            assert sorted(got) == ["action", "image", "position", "translation", "velocity"]
            for k in got:
                _same_bits(got[k], want[k], (k, n + 1))
    assert policy.pushes == pushes
    assert int(policy._fill.sum().item()) == 0                                  # cleared after the push that used it


def test_a_reset_refills_only_the_environments_named():
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    policy = ClosedLoopPolicy(_geometry(4, 1), _stats("float64"), n_envs=3, image_storage="uint8")
    low = np.zeros((3, 7))
    for n in range(7):
        if n == 5:
            policy.reset([1])
        policy.observe(np.full((3, 96, 96, 3), n, np.uint8), low[:, :2], low[:, 2:4], low[:, 4:])
    img = policy.batch()["image"]
    assert (img[:, :, 0, 0, 0] * 255).round().tolist() == [[3, 4, 5, 6], [5, 5, 5, 6], [3, 4, 5, 6]]
    assert bool((img == img[:, :, :1, :1, :1]).all())                          # every pixel of a frame moved


# ---- spdm_policy_unnormalize -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 2])
@pytest.mark.parametrize("H,inp_h", [(8, 0), (9, 1), (16, 4)])
@pytest.mark.parametrize("E", [1, 3, 130])
def test_unnormalize_equals_the_restatement_bit_for_bit(E, H, inp_h, D):
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    stats = _stats("float64")
    policy = ClosedLoopPolicy(_geometry(2, 1, pred=H - inp_h, inp=inp_h, D=D), stats, n_envs=E)
    rng = np.random.default_rng([E, H, inp_h, D])
    x_0 = rng.uniform(-1.2, 1.2, (E, 1, H, D)).astype(np.float32)
    tr = rng.uniform(-1.0, 1.0, (E, 2)).astype(np.float32)
    plan = policy.unnormalize(torch.from_numpy(x_0).cuda(), torch.from_numpy(tr).cuda())
    way, act = policy_ref.plan(x_0[:, 0], tr, stats, inp_h)
    assert way.shape == (E, H - inp_h, 2) and np.isfinite(way).all()
    _same_bits(plan.waypoints, way, "waypoints")
    if D >= 5:
        _same_bits(plan.actions, act, "actions")
    else:
        assert plan.actions is None and act is None


# ---- end to end --------------------------------------------------------------------------------------------------------------
M_OBS, M_PRED, M_STEP, SEED = 2, 15, 3, 11


@functools.lru_cache(maxsize=None)
def _model(kind):
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd.diffusion import load_model
    return load_model(kind, None, None, num_of_ddim_steps=6, model="UNet_FilmnoAttention", noise_steps=6, obs_horizon=M_OBS,
                      pred_horizon=M_PRED, inpaint_horizon=1, observation_dim=135, prediction_dim=5, step_size=M_STEP,
                      vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=64, weight_seed=3)


def _x_T(E, seed):
    return torch.rand(E, 1, M_PRED + 1, 5, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


@pytest.mark.parametrize("kind", ["DDPM", "DDIM"])
def test_plan_equals_sampling_the_host_built_batch_bit_for_bit(kind):
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    model, stats, E = _model(kind), _stats("float64"), 3
    policy = ClosedLoopPolicy(model, stats, n_envs=E, image_storage="uint8")
    assert (policy.obs_horizon, policy.pred_horizon, policy.inpaint_horizon, policy.step_size, policy.history) == (2, 15, 1, 3, 6)
    ref = policy_ref.History(E, policy.history)
    for obs in _observations(E, 9, "uint8", 77):                               # 9 observes wrap L = 6
        policy.observe(*obs)
        ref.push(*obs)
    x = _x_T(E, 5)
    plan = policy.plan(seed=SEED, x_T=x.clone())
    assert plan.x_0.shape == (E, 1, M_PRED + 1, 5) and plan.waypoints.shape == (E, M_PRED, 2) and plan.actions.shape == (E, M_PRED, 3)
    assert plan.waypoints.dtype == plan.actions.dtype == torch.float64 and plan.waypoints.is_cuda
    host = policy_ref.batch(ref, stats, M_STEP)
    uploaded = {k: torch.from_numpy(host[k]).cuda() for k in ("image", "position", "velocity", "action")}
    x_0 = model.sample(uploaded, batched=True, sharded=False, seed=SEED, x_T=x.clone())
    assert torch.isfinite(x_0).all() and torch.equal(plan.x_0, x_0)
    way, act = policy_ref.plan(x_0.cpu().numpy()[:, 0], host["translation"], stats, 1)
    _same_bits(plan.waypoints, way, "waypoints")
    _same_bits(plan.actions, act, "actions")
    assert not np.array_equal(way[0], way[1])                                  # the environments saw different observations


def test_a_repeated_plan_is_identical_and_replays_the_captured_graph():
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    model, E = _model("DDIM"), 3
    policy = ClosedLoopPolicy(model, _stats("float64"), n_envs=E, image_storage="uint8")
    for obs in _observations(E, 2, "uint8", 78):
        policy.observe(*obs)
    x = _x_T(E, 6)
    a = policy.plan(seed=SEED, x_T=x.clone())
    captures = model._engine.graph_captures
    b = policy.plan(seed=SEED, x_T=x.clone())
    assert model._engine.graph_captures == captures
    assert torch.equal(a.x_0, b.x_0) and torch.equal(a.waypoints, b.waypoints) and torch.equal(a.actions, b.actions)
    for obs in _observations(E, 3, "uint8", 79):                               # [::3] of a history of 6 reads entries 0 and 3:
        policy.observe(*obs)                                                    # three more steps bring a new observation there
    assert not torch.equal(policy.plan(seed=SEED, x_T=x.clone()).waypoints, a.waypoints)


# ---- error paths -------------------------------------------------------------------------------------------------------------
def test_the_policy_refuses_what_it_cannot_do():
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    policy = ClosedLoopPolicy(_geometry(2, 3), _stats("float64"), n_envs=2, image_storage="uint8")
    with pytest.raises(RuntimeError, match="observe"):
        policy.batch()
    with pytest.raises(RuntimeError, match="observe"):
        policy.plan()
    img, low = np.zeros((2, 96, 96, 3), np.uint8), np.zeros((2, 7))
    good = dict(img=img, position=low[:, :2], velocity=low[:, 2:4], action=low[:, 4:])
    for name, bad, exc in (("img", img[:1], ValueError), ("img", img.astype(np.float32), TypeError), ("img", img[:, :95], ValueError),
                           ("position", low[:, :3], ValueError), ("velocity", low[:1, :2], ValueError), ("action", low[:, :2], ValueError),
                           ("action", np.zeros((2, 3), np.complex64), TypeError)):
        with pytest.raises(exc, match=name):
            policy.observe(**{**good, name: bad})
    assert policy.pushes == 0
    policy.observe(**good)
    assert policy.batch()["image"].shape == (2, 2, 3, 96, 96)
    with pytest.raises(IndexError):
        policy.reset([2])
    with pytest.raises(ValueError, match="image_storage"):
        ClosedLoopPolicy(_geometry(2, 3), _stats("float64"), image_storage="auto")
    mixed = {**_stats("float64"), "velocity": {"min": _stats("float32")["velocity"]["min"], "max": _stats("float64")["velocity"]["max"]}}
    with pytest.raises(ValueError, match="velocity"):
        ClosedLoopPolicy(_geometry(2, 3), mixed)


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_the_command_line_replays_the_recorded_episodes(tmp_path):
    """python -m state_policy_diffusionmodel_amd.run_predictions on a checkpoint, hparams.yaml, STATS.pkl and arrays.npz written
    here (in process: the test starts nothing) against a ClosedLoopPolicy driven directly."""
    import yaml
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd import weights
    from state_policy_diffusionmodel_amd.diffusion import load_model
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    from state_policy_diffusionmodel_amd.run_predictions import main
    T, EVERY = 140, 20
    hp = dict(noise_steps=6, obs_horizon=M_OBS, pred_horizon=M_PRED, observation_dim=135, prediction_dim=5, learning_rate=1e-4,
              model="UNet_FilmnoAttention", noise_scheduler_type="linear", inpaint_horizon=1, step_size=M_STEP)
    sd = weights.random_state_dict(135 * M_OBS, seed=3, attention=False, model="UNet_FilmnoAttention", noise_steps=6)
    full = {"noise_estimator." + k: torch.from_numpy(np.array(v)) for k, v in weights.state_dict_to_numpy(sd).items()}
    full.update({"vision_encoder." + k: v for k, v in make_encoder_state_dict(7).items()})
    paths = {k: str(tmp_path / k) for k in ("epoch=0.ckpt", "hparams.yaml", "STATS.pkl", "arrays.npz", "report.json")}
    torch.save({"state_dict": full}, paths["epoch=0.ckpt"])
    with open(paths["hparams.yaml"], "w") as f:
        f.write(yaml.safe_dump(hp))
    stats = _stats("float64")
    with open(paths["STATS.pkl"], "wb") as f:
        pickle.dump([stats], f)
    g = np.load(GOLDEN)
    img = np.random.default_rng(5).integers(0, 256, (T, 96, 96, 3), dtype=np.uint8)
    np.savez(paths["arrays.npz"], position=g["position"], velocity=g["velocity"], action=g["action"], episode_ends=g["episode_ends"], img=img)
    report = main(["--model_name", "DDPM", "--checkpoint", paths["epoch=0.ckpt"], "--hparams", paths["hparams.yaml"], "--stats", paths["STATS.pkl"],
                   "--data", paths["arrays.npz"], "--replan_every", str(EVERY), "--seed", str(SEED), "--out", paths["report.json"]])
    back = json.load(open(paths["report.json"]))
    # episodes [0, 37), [37, 60), [60, 61), [61, 140): a plan on every 20th row of each
    want_rows = [0, 20, 37, 57, 60, 61, 81, 101, 121]
    ends = {0: 37, 20: 37, 37: 60, 57: 60, 60: 61}
    assert [p["row"] for p in back["plans"]] == want_rows and back["step_size"] == M_STEP and back["image_storage"] == "uint8"
    left = 0
    for p in back["plans"]:
        ahead = p["row"] + 1 + M_STEP * np.arange(M_PRED)                       # the rows of the 15 way-points
        inside = int((ahead < ends.get(p["row"], T)).sum())
        assert len(p["errors"]) == inside and p["left_out"] == M_PRED - inside and p["seconds"] > 0
        left += M_PRED - inside
    assert back["left_out"] == left > 0 and back == json.loads(json.dumps(report))
    assert len(back["mean_error"]) == M_PRED and back["mean_error"][0] > 0 and back["std_error"][0] >= 0
    # the first plan, computed directly: one observation fills the history, way-point j is compared with row 1 + 3 j
    policy = ClosedLoopPolicy(load_model("DDPM", paths["epoch=0.ckpt"], paths["hparams.yaml"], max_batch=1), stats, n_envs=1, image_storage="uint8")
    policy.observe(img[:1], g["position"][:1], g["velocity"][:1], g["action"][:1])
    way = policy.plan(seed=SEED, x_T=_x_T(1, SEED)).waypoints[0].cpu().numpy()
    rows = 1 + M_STEP * np.arange(M_PRED)
    rows = rows[rows < 37]
    d = g["position"][rows] - way[:len(rows)]
    assert back["plans"][0]["errors"] == np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).tolist()
