"""Planning from K candidates per environment on the GPU: spdm_policy_select against tests/ensemble_ref.py,
``sample(candidates=K)`` against the host-repeated batch, ``ClosedLoopPolicy.plan_candidates(candidates=K)`` against its manual composition,
and the command line's ``--candidates``.  The launch is float64 arithmetic rounded operation by operation in a fixed order plus
exact copies, and the sampler is compared with itself, so the tolerance is zero throughout."""
import functools
import json
import os
import pickle
import types

import numpy as np
import pytest
import torch

import ensemble_ref as er
import policy_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_small.npz")


@functools.lru_cache(maxsize=None)
def _stats():
    d = np.load(GOLDEN)
    return {"position": {"min": d["s5/pos_min"][()], "max": d["s5/pos_max"][()]},
            "velocity": {k: d["s5/vel_" + k].astype(np.float64) for k in ("min", "max")},
            "action": {k: d["s5/act_" + k].astype(np.float64) for k in ("min", "max")}}


def _pos():
    return float(_stats()["position"]["min"]), float(_stats()["position"]["max"])


def _bits_equal(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = np.count_nonzero(np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits))
    assert diff == 0, f"{what}: {diff} of {got.size} elements differ"


def _kernel_policy(E, H, D, inp_h):
    """A policy that samples nothing: what ``select`` reads of a model is its geometry."""
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    model = types.SimpleNamespace(obs_horizon=1, pred_horizon=H - inp_h, inpaint_horizon=inp_h, prediction_dim=D, step_size=1,
                                  device=torch.device("cuda", 0))
    return ClosedLoopPolicy(model, _stats(), n_envs=E)


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _check(policy, x, mode, cols, tr, what, guess=None, rows=0, stride=1):
    """One launch against the restatement, bit for bit; returns the launch's outputs."""
    E, K, H, D = x.shape
    inp_h = policy.inpaint_horizon
    want = er.select(x, er.COHERENT if mode == "coherent" else er.MEDOID, inp_h, cols, guess=guess, rows=rows, translation=tr,
                     pos_min=_pos()[0], pos_max=_pos()[1])
    d_guess = None if guess is None else _dev(np.repeat(guess, stride, axis=0))      # stride K: K identical rows per environment
    got = policy.select(_dev(x.reshape(E * K, 1, H, D)), K, mode, guess=d_guess, rows=rows, guess_row_stride=stride, cols=cols,
                        translation=_dev(tr))
    assert got[1].shape == (E, 1, H, D)
    _bits_equal(got[0], want[0], (what, "chosen"))
    _bits_equal(got[2], want[2], (what, "scores"))
    _bits_equal(got[1][:, 0], want[1], (what, "x0_out"))
    _bits_equal(got[3], want[3], (what, "spread"))
    return got


# ---- spdm_policy_select against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("H,inp_h", [(8, 0), (9, 1)])
@pytest.mark.parametrize("K", [1, 2, 5, 64])
@pytest.mark.parametrize("E", [1, 3, 130])
def test_the_kernel_equals_the_restatement(E, K, H, inp_h):
    P = H - inp_h
    for D, cols in ((2, 2), (5, 2), (5, 5)):
        policy = _kernel_policy(E, H, D, inp_h)
        rng = np.random.default_rng([E, K, H, inp_h, D, cols])
        x = rng.uniform(-1.2, 1.2, (E, K, H, D)).astype(np.float32)
        tr = rng.uniform(-1.0, 1.0, (E, 2)).astype(np.float32)
        guess = rng.uniform(-1.2, 1.2, (E, H, D)).astype(np.float32)
        what = (D, cols)
        first = _check(policy, x, "medoid", cols, tr, what + ("medoid",))
        for rows in sorted({1, P}):
            for stride in sorted({1, K}):
                _check(policy, x, "coherent", cols, tr, what + ("coherent", rows, stride), guess=guess, rows=rows, stride=stride)
        # exact ties: the last candidate repeats the first, and the guess is that candidate, so both score 0 and 0 is kept
        if K >= 2:
            x[:, K - 1] = x[:, 0]
            got = _check(policy, x, "medoid", cols, tr, what + ("medoid, tied",))
            assert torch.equal(got[2][:, 0], got[2][:, K - 1]) and not bool((got[0] == K - 1).any())
            got = _check(policy, x, "coherent", cols, tr, what + ("coherent, tied",), guess=np.ascontiguousarray(x[:, 0]), rows=P)
            assert bool((got[0] == 0).all()) and bool((got[2][:, 0] == 0).all())
        # two calls give the same bits
        twice = [policy.select(_dev(x.reshape(E * K, 1, H, D)), K, "medoid", cols=cols, translation=_dev(tr)) for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(*twice))
        assert first[2].shape == (E, K) and first[3].shape == (E, P)


def test_the_candidates_are_staged_or_read_in_place_with_the_same_bits():
    """The distance loops and the spread read a copy of the candidates' scored part in LDS when it fits and global memory when it
    does not.  K = 64 candidates of P = 51 rows and 5 columns are 64 x 255 floats, past the 64 KiB of a workgroup in either mode;
    cols = 2 of the same set (64 x 103 floats) fits in both: all four routes against the restatement."""
    E, K, H, inp_h, D = 2, 64, 53, 2, 5
    policy = _kernel_policy(E, H, D, inp_h)
    rng = np.random.default_rng(40)
    x = rng.uniform(-1.2, 1.2, (E, K, H, D)).astype(np.float32)
    tr = rng.uniform(-1.0, 1.0, (E, 2)).astype(np.float32)
    guess = rng.uniform(-1.2, 1.2, (E, H, D)).astype(np.float32)
    for cols in (5, 2):
        _check(policy, x, "medoid", cols, tr, ("large", cols))
        _check(policy, x, "coherent", cols, tr, ("large", cols), guess=guess, rows=H - inp_h - 3, stride=1)


def test_a_nan_score_never_wins_on_the_device():
    E, K, H, inp_h, D = 4, 5, 9, 1, 5
    policy = _kernel_policy(E, H, D, inp_h)
    rng = np.random.default_rng(41)
    x = rng.uniform(-1.2, 1.2, (E, K, H, D)).astype(np.float32)
    guess = rng.uniform(-1.2, 1.2, (E, H, D)).astype(np.float32)
    x[0, 0, 3, 1] = np.nan                                                   # environment 0: candidate 0
    x[1, :, 4, 0] = np.nan                                                   # environment 1: every candidate
    x[2, 2, 5, 0] = np.inf                                                   # environment 2: inf - inf inside d(2, 2)
    x[3, 1, 2, 4] = np.nan                                                   # environment 3: outside cols = 2
    for mode, kw in (("medoid", {}), ("coherent", dict(guess=guess, rows=H - inp_h))):
        with np.errstate(invalid="ignore"):                                  # inf - inf is meant
            want = er.select(x, er.COHERENT if mode == "coherent" else er.MEDOID, inp_h, 2, **kw)
        got = policy.select(_dev(x.reshape(E * K, 1, H, D)), K, mode, cols=2, **{k: (_dev(v) if k == "guess" else v) for k, v in kw.items()})
        scores = got[2].cpu().numpy()
        assert np.array_equal(np.isnan(scores), np.isnan(want[2])) and np.array_equal(scores[~np.isnan(scores)], want[2][~np.isnan(want[2])])
        assert got[0].cpu().tolist() == want[0].tolist() and got[3] is None
        assert got[0][1].item() == 0 and np.isfinite(scores[3]).all()
        assert np.array_equal(got[1][:, 0].cpu().numpy(), want[1], equal_nan=True)


# ---- sample(candidates=K) and plan_candidates(candidates=K) ----------------------------------------------------------------------------
M_OBS, M_PRED, M_STEP, N_STEPS, SEED = 2, 15, 3, 6, 11
H_, D_ = M_PRED + 1, 5


@functools.lru_cache(maxsize=None)
def _model(kind):
    """The test model of tests/test_gpu_policy.py."""
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd.diffusion import load_model
    return load_model(kind, None, None, num_of_ddim_steps=N_STEPS, model="UNet_FilmnoAttention", noise_steps=N_STEPS, obs_horizon=M_OBS,
                      pred_horizon=M_PRED, inpaint_horizon=1, observation_dim=135, prediction_dim=5, step_size=M_STEP,
                      vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=64, weight_seed=3)


def _x_T(rows, seed):
    return torch.rand(rows, 1, H_, D_, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _observations(E, pushes, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (E, 96, 96, 3), dtype=np.uint8), 30.0 * rng.standard_normal((E, 2)), 12.0 * rng.standard_normal((E, 2)),
             rng.uniform(-1.0, 1.0, (E, 3))) for _ in range(pushes)]


def _policy(kind="DDIM", E=3, pushes=9, seed=77):
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


def _np(t):
    return t.cpu().numpy()


def _candidates(x_all, E, K):
    return np.ascontiguousarray(_np(x_all)[:, 0].reshape(E, K, H_, D_))


def test_one_candidate_is_the_plan_of_before_bit_for_bit():
    from state_policy_diffusionmodel_amd.policy import CandidatePlan, Plan
    model, E = _model("DDIM"), 3
    a, b = _policy(), _policy()
    x = _x_T(E, 5)
    plain = a.plan(seed=SEED, x_T=x.clone())
    captures = model._engine.graph_captures
    one = b.plan_candidates(seed=SEED, x_T=x.clone(), candidates=1, select="medoid", cols=5)
    assert model._engine.graph_captures == captures                          # no additional graph captures
    assert torch.equal(one.x_0, plain.x_0) and torch.equal(one.waypoints, plain.waypoints) and torch.equal(one.actions, plain.actions)
    assert type(plain) is Plan and type(one) is CandidatePlan
    assert (one.candidates, one.selected_by, one.chosen, one.scores, one.spread) == (1, "", None, None, None)
    assert (one.steps, one.warm) == (plain.steps, plain.warm) == (N_STEPS, False) and b.last_selection is None
    batch = b.batch()
    kw = dict(batched=True, sharded=False, seed=SEED)
    assert torch.equal(model.sample(dict(batch), x_T=x.clone(), candidates=1, **kw), model.sample(dict(batch), x_T=x.clone(), **kw))


@pytest.mark.parametrize("kind", ["DDPM", "DDIM"])
def test_a_plan_from_five_candidates_is_sample_select_and_unnormalize(kind):
    model, stats, E, K = _model(kind), _stats(), 3, 5
    policy = _policy(kind)
    x = _x_T(E * K, 6)
    plan = policy.plan_candidates(seed=SEED, x_T=x.clone(), candidates=K)
    assert (plan.candidates, plan.selected_by, plan.steps, plan.warm) == (K, "medoid", N_STEPS, False)     # no previous plan
    assert plan.x_0.shape == (E, 1, H_, D_) and plan.chosen.shape == (E,) and plan.chosen.dtype == torch.int32
    assert plan.scores.shape == (E, K) and plan.spread.shape == (E, M_PRED) and plan.scores.dtype == plan.spread.dtype == torch.float64
    assert plan.chosen.is_cuda and plan.scores.is_cuda and plan.spread.is_cuda
    batch = policy.batch()
    kw = dict(batched=True, sharded=False, seed=SEED)
    x_all = model.sample(dict(batch), candidates=K, x_T=x.clone(), **kw)
    assert x_all.shape == (E * K, 1, H_, D_) and torch.isfinite(x_all).all()
    chosen = plan.chosen.cpu().tolist()
    for e in range(E):
        assert torch.equal(plan.x_0[e], x_all[e * K + chosen[e]]), e
    tr = _np(batch["translation"])
    want = er.select(_candidates(x_all, E, K), er.MEDOID, 1, 2, translation=tr, pos_min=_pos()[0], pos_max=_pos()[1])
    _bits_equal(plan.chosen, want[0], "chosen")
    _bits_equal(plan.scores, want[2], "scores")
    _bits_equal(plan.spread, want[3], "spread")
    assert (want[3] > 0).all()
    way, act = policy_ref.plan(want[1], tr, stats, 1)
    _bits_equal(plan.waypoints, way, "waypoints")
    _bits_equal(plan.actions, act, "actions")
    assert torch.equal(policy._prev_x0, plan.x_0)                             # the state is the chosen plan
    # the candidates of an environment differ, and the device-repeated batch is the host-repeated one
    cand = _candidates(x_all, E, K)
    assert all(not np.array_equal(cand[e, j], cand[e, k]) for e in range(E) for j in range(K) for k in range(j))
    repeated = {k: batch[k].repeat_interleave(K, dim=0) for k in ("image", "position", "velocity", "action")}
    assert torch.equal(model.sample(repeated, x_T=x.clone(), **kw), x_all)
    # x_T left out is drawn at (E K, 1, H, D)
    assert model.sample(dict(batch), candidates=K, **kw).shape == (E * K, 1, H_, D_)


def test_the_selection_follows_the_previous_plan_while_one_is_usable():
    model, E, K = _model("DDIM"), 3, 4
    policy = _policy()
    limit = (M_PRED - 1) * M_STEP
    obs = _observations(E, limit + 6, 80)
    x = _x_T(E * K, 7)
    T0 = policy.batch()["translation"].clone()
    first = policy.plan_candidates(seed=SEED, x_T=x.clone(), candidates=K, select="coherent")
    assert first.selected_by == "medoid" and policy.last_selection == {"scored_by": "medoid", "rows": 0, "cols": 2}
    for _ in range(M_STEP + 1):                                              # delta = 4: one whole row and a third
        policy.observe(*obs.pop())
    second = policy.plan_candidates(seed=SEED + 1, x_T=x.clone(), candidates=K, select="coherent", cols=5)
    rows = M_PRED - 1 - 1
    assert second.selected_by == "coherent" and policy.last_selection == {"scored_by": "coherent", "rows": rows, "cols": 5}
    assert (second.steps, second.warm) == (N_STEPS, False)
    batch = policy.batch()
    inp = model.prepare_inpaint_vectors(batch).contiguous()
    guess = policy.warm_start(first.x_0, T0, batch["translation"], inp, M_STEP + 1, 0.8, 0.6, SEED + 1, 1, return_parts=True)[1]
    x_all = model.sample(dict(batch), batched=True, sharded=False, candidates=K, seed=SEED + 1, x_T=x.clone())
    want = er.select(_candidates(x_all, E, K), er.COHERENT, 1, 5, guess=_np(guess), rows=rows, translation=_np(batch["translation"]),
                     pos_min=_pos()[0], pos_max=_pos()[1])
    _bits_equal(second.chosen, want[0], "chosen")
    _bits_equal(second.scores, want[2], "scores")
    _bits_equal(second.spread, want[3], "spread")
    _bits_equal(second.x_0[:, 0], want[1], "x_0")
    # 'medoid' and 'first' on a twin in the same state: the scores 'first' reports are the coherent ones, its plan candidate 0
    for select in ("medoid", "first"):
        twin = _policy()
        twin.plan_candidates(seed=SEED, x_T=x.clone(), candidates=K, select="coherent")
        for o in _observations(E, limit + 6, 80)[::-1][:M_STEP + 1]:
            twin.observe(*o)
        plan = twin.plan_candidates(seed=SEED + 1, x_T=x.clone(), candidates=K, select=select, cols=5)
        assert plan.selected_by == select
        if select == "first":
            assert plan.chosen.cpu().tolist() == [0] * E and torch.equal(plan.x_0, x_all[0::K])
            _bits_equal(plan.scores, want[2], "scores of 'first'")
            assert twin.last_selection["scored_by"] == "coherent"
        else:
            medoid = er.select(_candidates(x_all, E, K), er.MEDOID, 1, 5)
            _bits_equal(plan.chosen, medoid[0], "medoid chosen")
            _bits_equal(plan.scores, medoid[2], "medoid scores")
    # the last delta at which a predicted row still overlaps, then one past it, then a reset
    for _ in range(limit):
        policy.observe(*obs.pop())
    plan = policy.plan_candidates(seed=SEED, x_T=x.clone(), candidates=K)
    assert plan.selected_by == "coherent" and policy.last_selection["rows"] == 1
    for _ in range(limit + 1):
        policy.observe(*_observations(E, 1, 81)[0])
    assert policy.plan_candidates(seed=SEED, x_T=x.clone(), candidates=K).selected_by == "medoid"
    policy.observe(*obs.pop())
    assert policy.plan_candidates(seed=SEED, x_T=x.clone(), candidates=K).selected_by == "coherent"
    policy.reset([1])
    policy.observe(*obs.pop())
    assert policy.plan_candidates(seed=SEED, x_T=x.clone(), candidates=K).selected_by == "medoid"


def test_a_warm_plan_from_four_candidates():
    model, E, K, W = _model("DDIM"), 3, 4, 3
    policy = _policy()
    x = _x_T(E * K, 8)
    T0 = policy.batch()["translation"].clone()
    first = policy.plan_candidates(seed=SEED, x_T=x.clone(), candidates=K, warm_start=W)
    assert (first.steps, first.warm, first.selected_by) == (N_STEPS, False, "medoid")
    for o in _observations(E, M_STEP + 1, 82):
        policy.observe(*o)
    plan = policy.plan_candidates(seed=SEED + 1, candidates=K, warm_start=W)
    assert (plan.steps, plan.warm, plan.selected_by, plan.candidates) == (W, True, "coherent", K)
    batch = policy.batch()
    sa, sb = _level(model, N_STEPS - W)
    rep = lambda t: t.repeat_interleave(K, dim=0)  # noqa: E731
    inp = model.prepare_inpaint_vectors(batch).contiguous()
    x_start, guess, noise = policy.warm_start(rep(first.x_0), rep(T0), rep(batch["translation"]), rep(inp), M_STEP + 1, sa, sb, SEED + 1, 1,
                                              return_parts=True)
    assert guess.shape == (E * K, H_, D_) and torch.equal(guess[0::K], guess[K - 1::K])       # K identical rows per environment
    noise = _np(noise).reshape(E, K, H_, D_)
    assert all(not np.array_equal(noise[e, j], noise[e, k]) for e in range(E) for j in range(K) for k in range(j))
    x_all = model.sample(dict(batch), batched=True, sharded=False, candidates=K, seed=SEED + 1, x_T=x_start, start_step=N_STEPS - W)
    cand = _candidates(x_all, E, K)
    assert np.isfinite(cand).all()
    assert all(not np.array_equal(cand[e, j], cand[e, k]) for e in range(E) for j in range(K) for k in range(j))
    rows = M_PRED - 1 - 1
    want = er.select(cand, er.COHERENT, 1, 2, guess=np.ascontiguousarray(_np(guess)[0::K]), rows=rows, translation=_np(batch["translation"]),
                     pos_min=_pos()[0], pos_max=_pos()[1])
    _bits_equal(plan.chosen, want[0], "chosen")
    _bits_equal(plan.scores, want[2], "scores")
    _bits_equal(plan.spread, want[3], "spread")
    _bits_equal(plan.x_0[:, 0], want[1], "x_0")
    way, act = policy_ref.plan(want[1], _np(batch["translation"]), _stats(), 1)
    _bits_equal(plan.waypoints, way, "waypoints")
    _bits_equal(plan.actions, act, "actions")


# ---- error paths -------------------------------------------------------------------------------------------------------------
def test_plan_and_sample_refuse_what_they_cannot_do():
    model, E = _model("DDIM"), 3
    policy = _policy(pushes=1)
    for bad in (0, -1, 65, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="candidates"):
            policy.plan_candidates(seed=SEED, candidates=bad)
    for bad in ("best", "", None, 0):
        with pytest.raises(ValueError, match="select"):
            policy.plan_candidates(seed=SEED, candidates=4, select=bad)
    for bad in (1, 0, 6, 2.0, True, None):
        with pytest.raises(ValueError, match="cols"):
            policy.plan_candidates(seed=SEED, candidates=4, cols=bad)
    for shape in ((E, 1, H_, D_), (E * 4, H_, D_), (E * 4, 1, H_, D_ - 1), (E * 5, 1, H_, D_)):
        with pytest.raises(ValueError, match="x_T"):
            policy.plan_candidates(seed=SEED, candidates=4, x_T=torch.zeros(shape, device="cuda"))
    assert policy.plans == 0 and policy._prev_x0 is None
    batch = policy.batch()
    with pytest.raises(ValueError, match="x_T"):
        model.sample(dict(batch), batched=True, sharded=False, candidates=4, x_T=torch.zeros(E, 1, H_, D_, device="cuda"))
    with pytest.raises(ValueError, match="batched=True"):
        model.sample(dict(batch), candidates=4)
    with pytest.raises(ValueError, match="sample_history"):
        model.sample(dict(batch), "sample_history", batched=True, sharded=False, candidates=4)
    with pytest.raises(ValueError, match="mode"):
        policy.select(torch.zeros(E * 4, 1, H_, D_, device="cuda"), 4, "first")
    with pytest.raises(ValueError, match="x_0"):
        policy.select(torch.zeros(E * 4 + 1, 1, H_, D_, device="cuda"), 4)
    with pytest.raises(ValueError, match="guess"):
        policy.select(torch.zeros(E * 4, 1, H_, D_, device="cuda"), 4, "coherent", guess=torch.zeros(E, H_, D_, device="cuda"), rows=1,
                      guess_row_stride=4)
    with pytest.raises(RuntimeError, match="policy_select"):                  # the library's own refusal, through the binding
        policy.select(torch.zeros(E * 4, 1, H_, D_, device="cuda"), 4, "coherent", guess=torch.zeros(E, H_, D_, device="cuda"), rows=M_PRED + 1)
    assert _policy(E=1, pushes=1).plan_candidates(seed=SEED, candidates=64).scores.shape == (1, 64)      # the largest K: the model's max_batch


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_the_command_line_reports_the_selection(tmp_path):
    import yaml
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd import weights
    from state_policy_diffusionmodel_amd.run_predictions import main
    T, EVERY, N, K = 140, 20, 6, 4
    hp = dict(noise_steps=N, obs_horizon=M_OBS, pred_horizon=M_PRED, observation_dim=135, prediction_dim=5, learning_rate=1e-4,
              model="UNet_FilmnoAttention", noise_scheduler_type="linear", inpaint_horizon=1, step_size=M_STEP)
    sd = weights.random_state_dict(135 * M_OBS, seed=3, attention=False, model="UNet_FilmnoAttention", noise_steps=N)
    full = {"noise_estimator." + k: torch.from_numpy(np.array(v)) for k, v in weights.state_dict_to_numpy(sd).items()}
    full.update({"vision_encoder." + k: v for k, v in make_encoder_state_dict(7).items()})
    paths = {k: str(tmp_path / k) for k in ("epoch=0.ckpt", "hparams.yaml", "STATS.pkl", "arrays.npz", "many.json", "first.json")}
    torch.save({"state_dict": full}, paths["epoch=0.ckpt"])
    with open(paths["hparams.yaml"], "w") as f:
        f.write(yaml.safe_dump(hp))
    with open(paths["STATS.pkl"], "wb") as f:
        pickle.dump([_stats()], f)
    g = np.load(GOLDEN)
    img = np.random.default_rng(5).integers(0, 256, (T, 96, 96, 3), dtype=np.uint8)
    np.savez(paths["arrays.npz"], position=g["position"], velocity=g["velocity"], action=g["action"], episode_ends=g["episode_ends"], img=img)
    common = ["--model_name", "DDPM", "--checkpoint", paths["epoch=0.ckpt"], "--hparams", paths["hparams.yaml"], "--stats", paths["STATS.pkl"],
              "--data", paths["arrays.npz"], "--replan_every", str(EVERY), "--seed", str(SEED), "--candidates", str(K)]
    report = main(common + ["--out", paths["many.json"]])
    back = json.load(open(paths["many.json"]))
    assert back == json.loads(json.dumps(report))
    assert (back["candidates"], back["select"], back["select_cols"]) == (K, "coherent", 2)
    # episodes [0, 37), [37, 60), [60, 61), [61, 140): the first plan of each has no predecessor; replans come 20 rows = 6 rows and
    # two thirds of a plan later, so the previous plan still informs 15 - 6 - 1 = 8 rows
    rows = [0, 20, 37, 57, 60, 61, 81, 101, 121]
    cold_rows = {0, 37, 60, 61}
    assert [p["row"] for p in back["plans"]] == rows
    for p in back["plans"]:
        by = "medoid" if p["row"] in cold_rows else "coherent"
        assert (p["selected_by"], p["scored_by"], p["rows"]) == (by, by, 0 if by == "medoid" else 8), p
        assert 0 <= p["chosen"] < K and p["score"] >= 0 and len(p["spread"]) == M_PRED and min(p["spread"]) > 0 and p["seconds"] > 0, p
    assert len(back["mean_spread"]) == M_PRED and min(back["mean_spread"]) > 0
    jumps = [p["score"] / (8 * 2) for p in back["plans"] if p["row"] not in cold_rows]
    assert back["mean_jump"] == float(np.mean(jumps)) > 0
    # candidate 0 alone, scored alike
    first = main(common + ["--select", "first", "--out", paths["first.json"]])
    assert [p["chosen"] for p in first["plans"]] == [0] * len(rows) and {p["selected_by"] for p in first["plans"]} == {"first"}
    assert [p["scored_by"] for p in first["plans"]] == [p["scored_by"] for p in back["plans"]] and first["mean_jump"] > 0
    assert first["plans"][0]["spread"] == back["plans"][0]["spread"]          # the same candidates before the first choice
