"""Warm-started replanning on the GPU: spdm_policy_warm_start against tests/warm_start_ref.py, a suffix of the
sampling loop against the whole loop, ``ClosedLoopPolicy.plan(warm_start=K)`` against its manual composition, and the command
line's ``--warm_start``.  Everything but the drawn noise is an exact copy or a correctly rounded operation in a fixed order, so the
tolerance is zero; the drawn normals go through logf / sinf / cosf, for which tests/test_gpu_forward_process.py derives 1e-5."""
import functools
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch

import policy_ref
import warm_start_ref as ws

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_small.npz")
NOISE_TOL = 1e-5
SA, SB = float(np.float32(0.83059514)), float(np.float32(0.55688236))


@functools.lru_cache(maxsize=None)
def _stats():
    d = np.load(GOLDEN)
    return {"position": {"min": d["s5/pos_min"][()], "max": d["s5/pos_max"][()]},
            "velocity": {k: d["s5/vel_" + k].astype(np.float64) for k in ("min", "max")},
            "action": {k: d["s5/act_" + k].astype(np.float64) for k in ("min", "max")}}


def _bits_equal(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = np.count_nonzero(np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits))
    assert diff == 0, f"{what}: {diff} of {got.size} elements differ"


def _kernel_policy(E, H, D, inp_h, step_size):
    """A policy that samples nothing: what ``warm_start`` reads of a model is its geometry."""
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    model = types.SimpleNamespace(obs_horizon=1, pred_horizon=max(H - inp_h, 1), inpaint_horizon=inp_h, prediction_dim=D,
                                  step_size=step_size, device=torch.device("cuda", 0))
    return ClosedLoopPolicy(model, _stats(), n_envs=E)


def _inputs(E, H, D, inp_h, seed):
    rng = np.random.default_rng(seed)
    prev = rng.uniform(-1.2, 1.2, (E, H, D)).astype(np.float32)
    T0 = rng.uniform(-1.0, 1.0, (E, 2)).astype(np.float32)
    T1 = (T0 + rng.uniform(-0.05, 0.05, (E, 2))).astype(np.float32)
    inpaint = rng.uniform(-1.2, 1.2, (E, inp_h, D)).astype(np.float32) if inp_h > 0 else None
    return prev, T0, T1, inpaint


def _dev(x):
    return None if x is None else torch.from_numpy(x).cuda()


# ---- spdm_policy_warm_start against the restatement --------------------------------------------------------------------------
CASES = ([(1, 1, 2, 0, 1, 0, 0)] +                                          # degenerate
         [(3, 16, 5, 1, 3, delta, 0) for delta in (0, 3, 4, 44, 45, 1000)] +   # whole / fractional shift, last overlap, all held, far beyond
         [(5, 9, 5, 4, 5, 7, 0),                                            # H D = 45: the last Philox quad of a window is short
          (2, 8, 2, 0, 2, 3, 0),                                            # D = 2: no action columns
          (130, 32, 5, 10, 5, 50, 0),                                       # several workgroups, the real geometry
          (4, 16, 5, 1, 3, 4, 2 ** 32 - 2)])                                # the global environment index wraps


@pytest.mark.parametrize("E,H,D,inp_h,step_size,delta,env_offset", CASES)
def test_the_kernel_equals_the_restatement(E, H, D, inp_h, step_size, delta, env_offset):
    policy = _kernel_policy(E, H, D, inp_h, step_size)
    prev, T0, T1, inpaint = _inputs(E, H, D, inp_h, [E, H, D, inp_h, step_size, delta])
    seed, draw = 0x1234_5678_9ABC_DEF0 >> 2, 7
    args = (_dev(prev), _dev(T0), _dev(T1), _dev(inpaint), delta, SA, SB)
    x, guess, noise = policy.warm_start(*args, seed, draw, env_offset=env_offset, return_parts=True)
    assert x.shape == (E, 1, H, D) and guess.shape == noise.shape == (E, H, D)
    # the shifted, re-centred plan: bit for bit
    _bits_equal(guess, ws.guess(prev, T0, T1, delta, step_size), "guess")
    # the drawn noise: within the bound of this Box-Muller code
    z = noise.cpu().numpy()
    worst = float(np.abs(z - ws.draw(seed, draw, env_offset, E, H, D)).max())
    print(f"warm start {(E, H, D, inp_h, step_size, delta)}: drawn noise differs from the restatement by at most {worst:.3e}")
    assert np.isfinite(z).all() and worst <= NOISE_TOL
    # the iterate: the three-operation formula on the kernel's own guess and noise, then the in-painting
    _bits_equal(x[:, 0], ws.constrain(ws.add_noise(guess.cpu().numpy(), z, SA, SB), inpaint), "x")
    # the caller's noise: everything bit for bit, and the output may be the input
    given = np.random.default_rng(9).standard_normal((E, H, D)).astype(np.float32)
    d_given = _dev(given)
    x2, guess2, used = policy.warm_start(*args, seed, draw, env_offset=env_offset, noise=d_given, return_parts=True)
    want_x, want_g, _ = ws.warm_start(prev, T0, T1, inpaint, delta, step_size, SA, SB, noise=given)
    assert used.data_ptr() == d_given.data_ptr()
    _bits_equal(used, given, "noise given")
    _bits_equal(guess2, want_g, "guess with noise given")
    _bits_equal(x2[:, 0], want_x, "x with noise given")
    _bits_equal(policy.warm_start(*args, seed, draw, env_offset=env_offset, noise=d_given)[:, 0], want_x, "x alone")
    # a second call gives the same bits
    x3, guess3, noise3 = policy.warm_start(*args, seed, draw, env_offset=env_offset, return_parts=True)
    assert torch.equal(x3, x) and torch.equal(guess3, guess) and torch.equal(noise3, noise)
    _bits_equal(policy.warm_start(*args, seed, draw, env_offset=env_offset)[:, 0], x[:, 0].cpu().numpy(), "x without the parts")


def test_the_noise_depends_on_draw_seed_and_environment_and_shards_like_the_whole():
    E, H, D, inp_h, step_size, delta = 4, 16, 5, 1, 3, 4
    policy, half = _kernel_policy(E, H, D, inp_h, step_size), _kernel_policy(E // 2, H, D, inp_h, step_size)
    prev, T0, T1, inpaint = _inputs(E, H, D, inp_h, 21)
    args = (_dev(prev), _dev(T0), _dev(T1), _dev(inpaint), delta, SA, SB)
    x, _, z = policy.warm_start(*args, 11, 3, return_parts=True)
    for seed, draw in ((11, 4), (12, 3), (11 + 2 ** 32, 3)):
        assert not torch.equal(policy.warm_start(*args, seed, draw, return_parts=True)[2], z), (seed, draw)
    assert not torch.equal(z[0], z[1]) and not torch.equal(z[1], z[2])
    second = tuple(None if t is None else t[E // 2:].contiguous() for t in args[:4]) + args[4:]
    xh, _, zh = half.warm_start(*second, 11, 3, env_offset=E // 2, return_parts=True)
    assert torch.equal(zh, z[E // 2:]) and torch.equal(xh, x[E // 2:])


# ---- a suffix of the loop is the loop ----------------------------------------------------------------------------------------
M_OBS, M_PRED, M_STEP, N_STEPS, SEED = 2, 15, 3, 8, 11


@functools.lru_cache(maxsize=None)
def _model(kind):
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd.diffusion import load_model
    return load_model(kind, None, None, num_of_ddim_steps=N_STEPS, model="UNet_FilmnoAttention", noise_steps=N_STEPS, obs_horizon=M_OBS,
                      pred_horizon=M_PRED, inpaint_horizon=1, observation_dim=135, prediction_dim=5, step_size=M_STEP,
                      vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=64, weight_seed=3)


def _x_T(E, seed):
    return torch.rand(E, 1, M_PRED + 1, 5, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _observations(E, pushes, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (E, 96, 96, 3), dtype=np.uint8), 30.0 * rng.standard_normal((E, 2)), 12.0 * rng.standard_normal((E, 2)),
             rng.uniform(-1.0, 1.0, (E, 3))) for _ in range(pushes)]


def _policy(kind, E=3, pushes=9, seed=77):
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    policy = ClosedLoopPolicy(_model(kind), _stats(), n_envs=E, image_storage="uint8")
    for obs in _observations(E, pushes, seed):
        policy.observe(*obs)
    return policy


def _level(model, i0):
    """(sa, sb) of loop iteration i0 from the scheduler's own table: columns 1 and 0 of its row i0."""
    from state_policy_diffusionmodel_amd.diffusion import _as_spec
    spec = _as_spec(model.noise_scheduler)
    spec.set_timesteps(model.noise_steps)
    row = np.asarray(spec.coefficient_table(), dtype=np.float32)[i0]
    return float(row[1]), float(row[0])


@pytest.mark.parametrize("kind", ["DDPM", "DDIM"])
def test_a_suffix_of_the_loop_is_the_loop(kind):
    model, E = _model(kind), 3
    batch = _policy(kind).batch()
    x = _x_T(E, 5)
    kw = dict(batched=True, sharded=False, seed=SEED)
    hist = model.sample(dict(batch), "sample_history", x_T=x.clone(), **kw)
    assert len(hist) == N_STEPS + 1 and torch.equal(hist[0], x) and torch.isfinite(hist[N_STEPS]).all()
    whole = model.sample(dict(batch), x_T=x.clone(), **kw)
    assert torch.equal(whole, hist[N_STEPS])
    assert torch.equal(model.sample(dict(batch), x_T=x.clone(), start_step=0, **kw), whole)
    for i0 in (1, N_STEPS - 3, N_STEPS - 1):                                 # N - 3 replays the step graph, N - 1 is too short for it
        assert not torch.equal(hist[i0], hist[N_STEPS])
        assert torch.equal(model.sample(dict(batch), x_T=hist[i0].clone(), start_step=i0, **kw), whole), i0


# ---- plan(warm_start=K) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 2])
def test_a_warm_plan_is_the_kernel_and_a_suffix_of_the_loop(K):
    model, stats, E = _model("DDIM"), _stats(), 3
    policy, twin, cold_twin = _policy("DDIM"), _policy("DDIM"), _policy("DDIM")
    x = _x_T(E, 5)
    T0 = policy.batch()["translation"].clone()
    first = policy.plan(seed=SEED, x_T=x.clone(), warm_start=K)             # no previous plan: cold
    captures = model._engine.graph_captures
    assert (first.steps, first.warm) == (N_STEPS, False)
    cold = cold_twin.plan(seed=SEED, x_T=x.clone())
    assert (cold.steps, cold.warm) == (N_STEPS, False)
    assert torch.equal(first.x_0, cold.x_0) and torch.equal(first.waypoints, cold.waypoints) and torch.equal(first.actions, cold.actions)
    twin.plan(seed=SEED, x_T=x.clone(), warm_start=K)
    more = _observations(E, M_STEP + 1, 78)                                  # delta = 4: one whole row and a third
    for obs in more:
        policy.observe(*obs)
        twin.observe(*obs)
    warm = policy.plan(seed=SEED + 1, x_T=x.clone(), warm_start=K)          # x_T is ignored
    assert (warm.steps, warm.warm) == (K, True)
    if K >= 3:
        assert model._engine.graph_captures == captures                      # the suffix replays the graph the cold plan captured
    # the manual composition
    batch = policy.batch()
    sa, sb = _level(model, N_STEPS - K)
    inp = model.prepare_inpaint_vectors(batch).contiguous()
    x_start, guess, noise = policy.warm_start(first.x_0, T0, batch["translation"], inp, M_STEP + 1, sa, sb, SEED + 1, 1, return_parts=True)
    prev = first.x_0[:, 0].cpu().numpy()
    _bits_equal(guess, ws.guess(prev, T0.cpu().numpy(), batch["translation"].cpu().numpy(), M_STEP + 1, M_STEP), "guess")
    assert float(np.abs(noise.cpu().numpy() - ws.draw(SEED + 1, 1, 0, E, M_PRED + 1, 5)).max()) <= NOISE_TOL
    _bits_equal(x_start[:, 0], ws.constrain(ws.add_noise(guess.cpu().numpy(), noise.cpu().numpy(), sa, sb), inp.cpu().numpy()), "x_start")
    x_0 = model.sample(dict(batch), batched=True, sharded=False, seed=SEED + 1, x_T=x_start, start_step=N_STEPS - K)
    assert torch.isfinite(x_0).all() and torch.equal(warm.x_0, x_0)
    way, act = policy_ref.plan(x_0.cpu().numpy()[:, 0], batch["translation"].cpu().numpy(), stats, 1)
    _bits_equal(warm.waypoints, way, "waypoints")
    _bits_equal(warm.actions, act, "actions")
    assert not torch.equal(warm.x_0, policy.plan(seed=SEED + 1, x_T=x.clone()).x_0)      # and not what a cold plan gives
    # an identically driven twin gives the same bits
    again = twin.plan(seed=SEED + 1, warm_start=K)
    assert (again.steps, again.warm) == (K, True)
    assert torch.equal(again.x_0, warm.x_0) and torch.equal(again.waypoints, warm.waypoints) and torch.equal(again.actions, warm.actions)


def test_a_reset_or_a_long_gap_makes_the_next_plan_cold():
    E, K = 3, 3
    policy = _policy("DDIM")
    x = _x_T(E, 5)
    limit = (M_PRED - 1) * M_STEP                                            # the last delta at which a predicted row still overlaps
    obs = _observations(E, 2 * limit + 4, 79)
    assert not policy.plan(seed=SEED, x_T=x.clone(), warm_start=K).warm
    policy.observe(*obs.pop())
    assert policy.plan(seed=SEED, warm_start=K).warm
    policy.reset([1])                                                        # one environment: the loop serves all, so all plan cold
    policy.observe(*obs.pop())
    plan = policy.plan(seed=SEED, x_T=x.clone(), warm_start=K)
    assert (plan.steps, plan.warm) == (N_STEPS, False)
    for _ in range(limit):
        policy.observe(*obs.pop())
    plan = policy.plan(seed=SEED, warm_start=K)
    assert (plan.steps, plan.warm) == (K, True)
    for _ in range(limit + 1):
        policy.observe(*obs.pop())
    plan = policy.plan(seed=SEED, x_T=x.clone(), warm_start=K)
    assert (plan.steps, plan.warm) == (N_STEPS, False)
    assert policy.plans == 5
    policy.observe(*obs.pop())
    assert not policy.plan(seed=SEED, x_T=x.clone()).warm                    # without the argument a plan is cold ...
    assert policy.plan(seed=SEED, warm_start=K).warm                         # ... and the next one may start from it


def test_plan_refuses_a_warm_start_outside_the_loop():
    policy = _policy("DDIM", pushes=1)
    for bad in (0, N_STEPS + 1, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="warm_start"):
            policy.plan(seed=SEED, warm_start=bad)
    assert policy.plans == 0
    assert policy.plan(seed=SEED, warm_start=N_STEPS).steps == N_STEPS


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_the_command_line_reports_cold_and_warm_plans_side_by_side(tmp_path):
    import yaml
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd import weights
    from state_policy_diffusionmodel_amd.run_predictions import main
    T, EVERY, N, K = 140, 20, 6, 3
    hp = dict(noise_steps=N, obs_horizon=M_OBS, pred_horizon=M_PRED, observation_dim=135, prediction_dim=5, learning_rate=1e-4,
              model="UNet_FilmnoAttention", noise_scheduler_type="linear", inpaint_horizon=1, step_size=M_STEP)
    sd = weights.random_state_dict(135 * M_OBS, seed=3, attention=False, model="UNet_FilmnoAttention", noise_steps=N)
    full = {"noise_estimator." + k: torch.from_numpy(np.array(v)) for k, v in weights.state_dict_to_numpy(sd).items()}
    full.update({"vision_encoder." + k: v for k, v in make_encoder_state_dict(7).items()})
    paths = {k: str(tmp_path / k) for k in ("epoch=0.ckpt", "hparams.yaml", "STATS.pkl", "arrays.npz", "warm.json", "plain.json")}
    torch.save({"state_dict": full}, paths["epoch=0.ckpt"])
    with open(paths["hparams.yaml"], "w") as f:
        f.write(yaml.safe_dump(hp))
    with open(paths["STATS.pkl"], "wb") as f:
        pickle.dump([_stats()], f)
    g = np.load(GOLDEN)
    img = np.random.default_rng(5).integers(0, 256, (T, 96, 96, 3), dtype=np.uint8)
    np.savez(paths["arrays.npz"], position=g["position"], velocity=g["velocity"], action=g["action"], episode_ends=g["episode_ends"], img=img)
    common = ["--model_name", "DDPM", "--checkpoint", paths["epoch=0.ckpt"], "--hparams", paths["hparams.yaml"], "--stats", paths["STATS.pkl"],
              "--data", paths["arrays.npz"], "--replan_every", str(EVERY), "--seed", str(SEED)]
    report = main(common + ["--warm_start", str(K), "--out", paths["warm.json"]])
    back = json.load(open(paths["warm.json"]))
    assert back == json.loads(json.dumps(report)) and back["warm_start"] == K
    # episodes [0, 37), [37, 60), [60, 61), [61, 140): the first plan of each is cold, the replans 20 rows later are warm
    rows = [0, 20, 37, 57, 60, 61, 81, 101, 121]
    cold_rows = {0, 37, 60, 61}
    assert [p["row"] for p in back["plans"]] == rows
    for p in back["plans"]:
        assert p["warm"] is (p["row"] not in cold_rows) and p["steps"] == (K if p["warm"] else N) and p["seconds"] > 0, p
    assert back["seconds_cold"] > 0 and back["seconds_warm"] > 0
    for name in ("cold", "warm"):
        mean, std = back["mean_error_" + name], back["std_error_" + name]
        assert len(mean) == len(std) == M_PRED and mean[0] > 0 and std[0] >= 0, name
    # without the flag: the report of before, with none of the new keys, and the cold plans are the same plans
    plain = main(common + ["--out", paths["plain.json"]])
    assert plain == json.load(open(paths["plain.json"]))
    assert sorted(plain) == sorted(["model_name", "obs_horizon", "pred_horizon", "step_size", "replan_every", "seed", "image_storage", "plans",
                                    "left_out", "mean_error", "std_error"])
    assert [p["row"] for p in plain["plans"]] == rows
    for p, q in zip(plain["plans"], back["plans"]):
        assert sorted(p) == ["episode_end", "errors", "left_out", "row", "seconds"]
        assert (p["episode_end"], p["left_out"]) == (q["episode_end"], q["left_out"])
        assert (p["errors"] == q["errors"]) is (p["row"] in cold_rows), p["row"]
