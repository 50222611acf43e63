"""DPM-Solver++ (2M) on the GPU: spdm_solver_step against the float32 restatement of tests/solver_ref.py bit for
bit, whole SPDM_DPMPP_2M trajectories against the oracle networks driven by the restatement's loop (tolerance 1e-4, the
project's trajectory bar), what a session keeps and forgets, and the facade.  The update is five correctly rounded float32
operations in a fixed order, so the kernel's tolerance is zero."""
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

import solver_ref as R
from oracle.unet_film_ref import unet_film_forward
from state_policy_diffusionmodel_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_small.npz")


def _bits_equal(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    got, want = got.reshape(want.shape), np.ascontiguousarray(want)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    diff = np.count_nonzero(np.ascontiguousarray(got).view(np.uint32) != want.view(np.uint32))
    assert diff == 0, f"{what}: {diff} of {got.size} elements differ"


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- spdm_solver_step against the restatement --------------------------------------------------------------------------------
# T = 20, n = 6: rows 0 and 5 are first order by construction, rows 1 .. 4 second order
STEPS = [(0, 0, True), (2, -1, False), (2, 2, True), (2, 1, False), (5, -1, True)]      # (step, first, runs first order)


# (B, H, D): 135 elements, no multiple of 256; 336, more than one workgroup.  inp_h 0, 1 and H, broadcast and per sample
KERNEL_CASES = [(B, H, D, inp_h, per_sample) for B, H, D in ((3, 9, 5), (7, 16, 3)) for inp_h in (0, 1, H) for per_sample in (False, True)
                if inp_h or not per_sample]


@pytest.mark.parametrize("B,H,D,inp_h,per_sample", KERNEL_CASES)
def test_the_kernel_equals_the_restatement(B, H, D, inp_h, per_sample):
    from state_policy_diffusionmodel_amd.engine import solver_step
    n = 6
    _, rows = R.table32(20, n)
    assert [bool(r[5] == 0) for r in rows] == [True, False, False, False, False, True]
    rng = np.random.default_rng([B, H, D, inp_h, int(per_sample)])
    coef = _dev(rows)
    inpaint = rng.uniform(-1.2, 1.2, (B, inp_h, D) if per_sample else (inp_h, D)).astype(np.float32) if inp_h else None
    d_inpaint = _dev(inpaint)
    for step, first, first_order in STEPS:
        for with_history in (True, False):
            eps = rng.standard_normal((B, H, D)).astype(np.float32)
            x = rng.uniform(-1.5, 1.5, (B, H, D)).astype(np.float32)
            x0_prev = rng.uniform(-1.5, 1.5, (B, H, D)).astype(np.float32)
            want_x, want_x0 = R.step(rows[step], eps, x, x0_prev, first=(step == first), inpaint=inpaint)
            plain, _ = R.step(rows[step], eps, x, x0_prev, first=True)
            assert (want_x[:, inp_h:] == plain[:, inp_h:]).all() == (first_order or inp_h == H)      # the case is what it claims to be
            d_eps, d_x, d_prev = _dev(eps), _dev(x), _dev(x0_prev)
            words = torch.tensor([77, 77, 0], dtype=torch.int32, device="cuda")
            hist = torch.full((n + 1, B, H, D), 123.0, device="cuda") if with_history else None
            solver_step(d_eps, d_x, d_prev, coef, step, first, words, inpaint=d_inpaint, history=hist)
            what = f"step {step} first {first} history {with_history}"
            _bits_equal(d_x, want_x, "x, " + what)
            _bits_equal(d_prev, want_x0, "x0, " + what)
            _bits_equal(d_eps, eps, "eps, " + what)
            assert words.tolist() == [step, first, 0], what
            if with_history:
                _bits_equal(hist[step + 1], want_x, "history row, " + what)
                rest = torch.cat([hist[:step + 1], hist[step + 2:]])
                assert bool((rest == 123.0).all()), what


def test_a_non_finite_eps_sets_the_flag_and_a_finite_one_leaves_it():
    from state_policy_diffusionmodel_amd.engine import solver_step
    B, H, D, n = 3, 9, 5, 6
    _, rows = R.table32(20, n)
    rng = np.random.default_rng(3)
    eps = rng.standard_normal((B, H, D)).astype(np.float32)
    x = rng.uniform(-1.5, 1.5, (B, H, D)).astype(np.float32)
    x0_prev = rng.uniform(-1.5, 1.5, (B, H, D)).astype(np.float32)
    inpaint = rng.uniform(-1, 1, (1, D)).astype(np.float32)
    words = torch.zeros(3, dtype=torch.int32, device="cuda")
    d_x, d_prev = _dev(x), _dev(x0_prev)
    solver_step(_dev(eps), d_x, d_prev, _dev(rows), 2, -1, words, inpaint=_dev(inpaint))
    assert words.tolist() == [2, -1, 0]
    bad = eps.copy()
    bad[1, H - 1, 2] = np.nan
    d_x, d_prev = _dev(x), _dev(x0_prev)
    solver_step(_dev(bad), d_x, d_prev, _dev(rows), 2, -1, words, inpaint=_dev(inpaint))
    assert words.tolist() == [2, -1, 1]
    want_x, _ = R.step(rows[2], eps, x, x0_prev, first=False, inpaint=inpaint)
    got = d_x.cpu().numpy()
    assert np.isnan(got[1, H - 1, 2]) and np.isnan(d_prev.cpu().numpy()[1, H - 1, 2])
    mask = np.ones((B, H, D), dtype=bool)
    mask[1, H - 1, 2] = False
    assert np.array_equal(got[mask].view(np.uint32), want_x[mask].view(np.uint32))
    solver_step(_dev(eps), _dev(x), _dev(x0_prev), _dev(rows), 3, -1, words, inpaint=_dev(inpaint))
    assert words.tolist() == [3, -1, 1]                                      # the flag is only ever set


# ---- whole trajectories against the oracle networks --------------------------------------------------------------------------
B_, H_, D_ = 2, 16, 3
MODELS = ("UNet_Film", "UNet_FilmnoAttention", "UNet")
GRIDS = ((20, 6), (100, 16))                                                 # the final step lower order / second order


@functools.lru_cache(maxsize=None)
def _weights(model):
    if model == "UNet":
        return random_state_dict(20, seed=0, model="UNet", noise_steps=100)
    return random_state_dict(14, seed=5, attention=(model == "UNet_Film"))


@functools.lru_cache(maxsize=None)
def _inputs(model):
    g = torch.Generator().manual_seed(9)
    cond = torch.randn(B_, 1, 10, 2, generator=g) if model == "UNet" else torch.randn(B_, 1, 2, 7, generator=g)
    x_T = torch.rand(B_, 1, H_, D_, generator=g)
    inpaint = torch.rand(B_, 1, 1, D_, generator=g) * 2 - 1
    other = torch.rand(B_, 1, H_, D_, generator=g)
    return cond, x_T, inpaint, other


def _oracle(model):
    sd, (cond, _, _, _) = _weights(model), _inputs(model)
    if model == "UNet":
        from simple_unet_ref import simple_unet_forward
        net = lambda x, t: simple_unet_forward(sd, x, t, cond)
    else:
        net = lambda x, t: unet_film_forward(sd, x, t, cond, attention=(model == "UNet_Film"))

    def eps(x, t):
        with torch.no_grad():
            out = net(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).reshape(B_, 1, H_, D_), torch.tensor([t]))
        return out.reshape(B_, H_, D_).numpy()
    return eps


@functools.lru_cache(maxsize=None)
def _reference(model, T, n, begin=0):
    """The restatement's loop (float32 steps) around the oracle network, computed once per case: x_T and the iterates.
    ``begin > 0``: a new loop from iterate ``begin`` of the whole one, first order there."""
    _, x_T, inpaint, _ = _inputs(model)
    ts, rows = R.table32(T, n)
    x = x_T.numpy().reshape(B_, H_, D_) if begin == 0 else _reference(model, T, n)[begin]
    out = R.loop(rows, ts, _oracle(model), x, begin=begin, inpaint=inpaint.numpy().reshape(B_, 1, D_), dtype=np.float32)
    return [x] + out


def _engine(model, T=100, max_batch=B_):
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    if model == "UNet":
        eng = SpdmEngine(H_, D_, 20, max_batch=max_batch, model="UNet", num_train_timesteps=101)
    else:
        eng = SpdmEngine(H_, D_, 14, max_batch=max_batch, attention=(model == "UNet_Film"), num_train_timesteps=T)
    eng.load_state_dict(_weights(model))
    return eng


def _solver(T, n, **options):
    from state_policy_diffusionmodel_amd.schedulers import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(num_train_timesteps=T, **options)
    s.set_timesteps(n)
    return s


@pytest.mark.parametrize("T,n", GRIDS)
@pytest.mark.parametrize("model", MODELS)
def test_trajectories_match_the_oracle_driven_by_the_restatement(model, T, n):
    cond, x_T, inpaint, _ = _inputs(model)
    want = np.stack(_reference(model, T, n))
    eng = _engine(model)
    try:
        before = eng.device_bytes
        eng.set_scheduler(_solver(T, n))
        assert eng.kind == 2 and eng.n_steps == n
        assert eng.device_bytes > before                                     # the x0 buffer comes with the first such schedule ...
        grown = eng.device_bytes
        eng.set_scheduler(_solver(T, n))
        assert eng.device_bytes == grown                                     # ... and only with the first
        x0, hist = eng.sample(cond.cuda(), x_T.cuda(), inpaint=inpaint.cuda(), history=True)
        got = hist.cpu().numpy().reshape(n + 1, B_, H_, D_)
        err = np.abs(got - want).reshape(n + 1, -1).max(axis=1)
        print(f"{model} T = {T} n = {n}: max |iterate - reference| per iterate = {np.array2string(err, precision=2)}")
        assert float(err.max()) <= TOL, err
        assert torch.equal(x0, hist[n]) and np.array_equal(got[0], want[0])
        assert np.array_equal(got[1:, :, :1], np.broadcast_to(inpaint.numpy().reshape(B_, 1, D_), (n, B_, 1, D_)))
        if model == "UNet_Film":
            # the same network on the other route: sa6 leaves its features, out_step writes eps, the solver's launch follows
            eng.set_switch("SPDM_NO_SA_OUTC", True)
            _, hist = eng.sample(cond.cuda(), x_T.cuda(), inpaint=inpaint.cuda(), history=True)
            err = np.abs(hist.cpu().numpy().reshape(n + 1, B_, H_, D_) - want).reshape(n + 1, -1).max(axis=1)
            print(f"{model} T = {T} n = {n}, eps from out_step: max |iterate - reference| = {float(err.max()):.2e}")
            assert float(err.max()) <= TOL, err
    finally:
        eng.close()


@pytest.mark.parametrize("model", ["UNet_Film", "UNet_FilmnoAttention"])
def test_a_suffix_starts_first_order(model):
    """``start_step = i0`` is a new session: it equals the restatement that starts first order at i0, not the whole loop's tail."""
    T, n, i0 = 100, 16, 13
    cond, _, inpaint, _ = _inputs(model)
    whole, suffix = _reference(model, T, n), _reference(model, T, n, begin=i0)
    assert len(suffix) == n - i0 + 1 and float(np.abs(suffix[-1] - whole[-1]).max()) > 10 * TOL      # the two ends are told apart
    eng = _engine(model)
    try:
        eng.set_scheduler(_solver(T, n))
        x_i0 = torch.from_numpy(whole[i0]).reshape(B_, 1, H_, D_).cuda()
        got = eng.sample(cond.cuda(), x_i0, inpaint=inpaint.cuda(), start_step=i0).cpu().numpy().reshape(B_, H_, D_)
        err = float(np.abs(got - suffix[-1]).max())
        print(f"{model}: suffix from {i0}: max |x_0 - reference| = {err:.2e}; whole loop's tail is {np.abs(got - whole[-1]).max():.2e} away")
        assert err <= TOL
    finally:
        eng.close()


# ---- what a session keeps and what it forgets --------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["UNet_Film", "UNet_FilmnoAttention"])
def test_pieces_graphs_and_sessions(model):
    from state_policy_diffusionmodel_amd.schedulers import DDIMScheduler
    T, n = 100, 16
    cond, x_T, inpaint, other = (t.cuda() for t in _inputs(model))
    kw = dict(inpaint=inpaint)
    eng = _engine(model)
    try:
        before = eng.device_bytes
        eng.set_scheduler(_solver(T, n))
        # the timesteps and the table, as for any schedule, and with the first solver schedule two (max_batch,H,D) buffers and a word
        assert eng.device_bytes - before == 28 * n + 2 * 4 * B_ * H_ * D_ + 4
        whole, hist = eng.sample(cond, x_T, history=True, **kw)
        assert eng.graph_captures >= 1
        # two pieces of one session are the whole run: the second continues the history
        for cut in (3, 1, n - 1):
            eng.sample_begin(cond, x_T, **kw)
            eng.sample_run(0, cut)
            eng.sample_run(cut, n)
            assert torch.equal(eng.sample_result(), whole), cut
        eng.sample_begin(cond, x_T, **kw)
        for i in range(n):
            eng.sample_run(i, i + 1)
        assert torch.equal(eng.sample_result(), whole)
        # a piece that does not continue the session's last step starts first order: not the whole run
        eng.sample_begin(cond, x_T, **kw)
        eng.sample_run(0, 3)
        first_three = eng.sample_result()
        assert torch.equal(first_three, hist[3])
        eng.sample_begin(cond, first_three, **kw)
        eng.sample_run(3, n)
        assert not torch.equal(eng.sample_result(), whole)
        # graph replay equals plain launches
        eng.set_switch("SPDM_NO_GRAPH", True)
        plain, plain_hist = eng.sample(cond, x_T, history=True, **kw)
        eng.set_switch("SPDM_NO_GRAPH", False)
        assert torch.equal(plain, whole) and torch.equal(plain_hist, hist)
        # nothing of the x0 buffer survives a session: a second x_T on this engine equals a fresh engine's
        second = eng.sample(cond, other, **kw)
        again = eng.sample(cond, x_T, **kw)
        assert torch.equal(again, whole) and not torch.equal(second, whole)
        # and DDIM after it is DDIM
        ddim = DDIMScheduler(num_train_timesteps=T)
        ddim.set_timesteps(n)
        eng.set_scheduler(ddim)
        ddim_after = eng.sample(cond, x_T, **kw)
    finally:
        eng.close()
    fresh = _engine(model)
    try:
        fresh.set_scheduler(_solver(T, n))
        assert torch.equal(fresh.sample(cond, other, **kw), second)
    finally:
        fresh.close()
    fresh = _engine(model)
    try:
        before = fresh.device_bytes
        fresh.set_scheduler(ddim)
        assert fresh.device_bytes - before == 28 * n                         # a handle that never sees the solver allocates as before
        assert torch.equal(fresh.sample(cond, x_T, **kw), ddim_after)
    finally:
        fresh.close()


# ---- the facade --------------------------------------------------------------------------------------------------------------
M_OBS, M_PRED, M_STEP, T_TRAIN, N_STEPS, SEED = 2, 15, 3, 20, 6, 11


@functools.lru_cache(maxsize=None)
def _stats():
    d = np.load(GOLDEN)
    return {"position": {"min": d["s5/pos_min"][()], "max": d["s5/pos_max"][()]},
            "velocity": {k: d["s5/vel_" + k].astype(np.float64) for k in ("min", "max")},
            "action": {k: d["s5/act_" + k].astype(np.float64) for k in ("min", "max")}}


def _load(**kw):
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd.diffusion import load_model
    return load_model("DDPM", None, None, model="UNet_FilmnoAttention", noise_steps=T_TRAIN, obs_horizon=M_OBS, pred_horizon=M_PRED,
                      inpaint_horizon=1, observation_dim=135, prediction_dim=5, step_size=M_STEP,
                      vision_encoder_state_dict=make_encoder_state_dict(7), max_batch=8, weight_seed=3, **kw)


@functools.lru_cache(maxsize=None)
def _model():
    return _load(solver_steps=N_STEPS)


def _observations(E, pushes, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (E, 96, 96, 3), dtype=np.uint8), 30.0 * rng.standard_normal((E, 2)), 12.0 * rng.standard_normal((E, 2)),
             rng.uniform(-1.0, 1.0, (E, 3))) for _ in range(pushes)]


def _policy(model, E=3, pushes=9, seed=77):
    from state_policy_diffusionmodel_amd.policy import ClosedLoopPolicy
    policy = ClosedLoopPolicy(model, _stats(), n_envs=E, image_storage="uint8")
    for obs in _observations(E, pushes, seed):
        policy.observe(*obs)
    return policy


def _x_T(E, seed):
    return torch.rand(E, 1, M_PRED + 1, 5, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _facade_reference(model, batch, x, begin):
    """The restatement's loop around the oracle network on the model's own weights and conditioning, from iterate x."""
    sd = model.noise_estimator.state_dict()
    cond = model.prepare_obs_cond_vectors(dict(batch)).unsqueeze(1).cpu()
    inpaint = model.prepare_inpaint_vectors(dict(batch)).cpu().numpy()
    E = cond.shape[0]
    ts, rows = R.table32(T_TRAIN, N_STEPS)

    def eps(v, t):
        with torch.no_grad():
            out = unet_film_forward(sd, torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).reshape(E, 1, M_PRED + 1, 5),
                                    torch.tensor([t]), cond, attention=False)
        return out.reshape(E, M_PRED + 1, 5).numpy()
    return R.loop(rows, ts, eps, x.cpu().numpy().reshape(E, M_PRED + 1, 5), begin=begin, inpaint=inpaint, dtype=np.float32)


def test_assigning_the_scheduler_is_load_model_with_solver_steps():
    from state_policy_diffusionmodel_amd.schedulers import DPMSolverMultistepScheduler
    model, E = _model(), 3
    assert isinstance(model.noise_scheduler, DPMSolverMultistepScheduler) and model.noise_steps == N_STEPS
    batch = _policy(model).batch()
    x = _x_T(E, 5)
    kw = dict(batched=True, sharded=False, seed=SEED)
    x_0 = model.sample(dict(batch), x_T=x.clone(), **kw)
    hist = model.sample(dict(batch), "sample_history", x_T=x.clone(), **kw)
    assert len(hist) == N_STEPS + 1 and torch.equal(hist[0], x) and torch.equal(hist[N_STEPS], x_0) and torch.isfinite(x_0).all()
    want = _facade_reference(model, batch, x, 0)
    err = max(float(np.abs(h.cpu().numpy().reshape(w.shape) - w).max()) for h, w in zip(hist[1:], want))
    print(f"facade: max |iterate - reference| over {N_STEPS} iterates = {err:.2e}")
    assert err <= TOL
    assigned = _load()                                                       # generate.py's idiom
    assigned.noise_scheduler = DPMSolverMultistepScheduler(num_train_timesteps=assigned.noise_steps)
    assigned.noise_steps = N_STEPS
    assert torch.equal(assigned.sample(dict(batch), x_T=x.clone(), **kw), x_0)


def test_a_warm_plan_runs_its_steps_first_order_first():
    model, E, K = _model(), 3, 3
    policy = _policy(model)
    x = _x_T(E, 5)
    T0 = policy.batch()["translation"].clone()
    first = policy.plan(seed=SEED, x_T=x.clone(), warm_start=K)
    assert (first.steps, first.warm) == (N_STEPS, False)
    for obs in _observations(E, M_STEP + 1, 78):
        policy.observe(*obs)
    warm = policy.plan(seed=SEED + 1, warm_start=K)
    assert (warm.steps, warm.warm) == (K, True)
    batch = policy.batch()
    row = R.table32(T_TRAIN, N_STEPS)[1][N_STEPS - K]
    assert policy._noise_level(N_STEPS - K) == (float(row[1]), float(row[0]))      # columns 0 and 1 keep their meaning
    inp = model.prepare_inpaint_vectors(batch).contiguous()
    x_start = policy.warm_start(first.x_0, T0, batch["translation"], inp, M_STEP + 1, float(row[1]), float(row[0]), SEED + 1, 1)
    x_0 = model.sample(dict(batch), batched=True, sharded=False, seed=SEED + 1, x_T=x_start, start_step=N_STEPS - K)
    assert torch.isfinite(x_0).all() and torch.equal(warm.x_0, x_0)
    want = _facade_reference(model, batch, x_start, N_STEPS - K)
    assert len(want) == K
    err = float(np.abs(x_0.cpu().numpy().reshape(want[-1].shape) - want[-1]).max())
    print(f"warm plan: max |x_0 - reference| = {err:.2e}")
    assert err <= TOL


def test_the_command_line_takes_solver_steps(tmp_path):
    import yaml
    from oracle.encoder_ref import make_encoder_state_dict
    from state_policy_diffusionmodel_amd import weights
    from state_policy_diffusionmodel_amd.run_predictions import main
    T, EVERY = 140, 40
    hp = dict(noise_steps=T_TRAIN, obs_horizon=M_OBS, pred_horizon=M_PRED, observation_dim=135, prediction_dim=5, learning_rate=1e-4,
              model="UNet_FilmnoAttention", noise_scheduler_type="linear", inpaint_horizon=1, step_size=M_STEP)
    sd = weights.random_state_dict(135 * M_OBS, seed=3, attention=False, model="UNet_FilmnoAttention", noise_steps=T_TRAIN)
    full = {"noise_estimator." + k: torch.from_numpy(np.array(v)) for k, v in weights.state_dict_to_numpy(sd).items()}
    full.update({"vision_encoder." + k: v for k, v in make_encoder_state_dict(7).items()})
    paths = {k: str(tmp_path / k) for k in ("epoch=0.ckpt", "hparams.yaml", "STATS.pkl", "arrays.npz", "solver.json")}
    torch.save({"state_dict": full}, paths["epoch=0.ckpt"])
    with open(paths["hparams.yaml"], "w") as f:
        f.write(yaml.safe_dump(hp))
    with open(paths["STATS.pkl"], "wb") as f:
        pickle.dump([_stats()], f)
    g = np.load(GOLDEN)
    img = np.random.default_rng(5).integers(0, 256, (T, 96, 96, 3), dtype=np.uint8)
    np.savez(paths["arrays.npz"], position=g["position"], velocity=g["velocity"], action=g["action"], episode_ends=g["episode_ends"], img=img)
    report = main(["--model_name", "DDPM", "--checkpoint", paths["epoch=0.ckpt"], "--hparams", paths["hparams.yaml"], "--stats", paths["STATS.pkl"],
                   "--data", paths["arrays.npz"], "--replan_every", str(EVERY), "--seed", str(SEED), "--solver_steps", str(N_STEPS),
                   "--out", paths["solver.json"]])
    back = json.load(open(paths["solver.json"]))
    assert back == json.loads(json.dumps(report))
    assert back["solver"] == {"name": "dpmsolver++2m", "steps": N_STEPS}
    assert sorted(back) == sorted(["model_name", "obs_horizon", "pred_horizon", "step_size", "replan_every", "seed", "image_storage", "plans",
                                   "left_out", "mean_error", "std_error", "solver"])
    assert len(back["plans"]) >= 4 and all(p["seconds"] > 0 and np.isfinite(p["errors"]).all() for p in back["plans"])
    assert len(back["mean_error"]) == M_PRED and back["mean_error"][0] > 0
