"""A numpy restatement of the observation noise (state_policy_diffusionmodel_amd/noising.py, csrc/obs_noise.hip), written from
its description in include/spdm.h on oracle.philox_ref.philox4x32_10, and the host arm of the robustness evaluation.  numpy
rounds each float32 array operation on its own, so these are the kernel's bits.  Test support only."""
import numpy as np

from oracle.philox_ref import philox4x32_10

KEYS = ("image", "position", "velocity", "action")                  # Philox purposes 4, 5, 6, 7


def words(seed, draw, purpose, row_offset, n_rows, inner):
    """(n_rows, inner) uint32: element e of row r is word e % 4 of Philox(counter (e // 4, row_offset + r, draw, purpose))."""
    nq = (inner + 3) // 4
    q = np.arange(nq, dtype=np.uint32)[None, :]
    row = (np.uint64(row_offset) + np.arange(n_rows, dtype=np.uint64)).astype(np.uint32)[:, None]
    w = philox4x32_10(q, row, np.uint32(draw), np.uint32(purpose), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack(w, axis=-1).reshape(n_rows, nq * 4)[:, :inner]


def uniforms(w):
    """float32 (w >> 8) 2^-24: exact, in [0, 1)."""
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def perturb(src, alpha, *, seed, draw, purpose, row_offset=0):
    """``src`` (n_rows, inner) float32 -> src + alpha u: the product rounded to float32, then the sum."""
    src = np.asarray(src)
    assert src.dtype == np.float32 and src.ndim == 2
    p = np.float32(alpha) * uniforms(words(seed, draw, purpose, row_offset, *src.shape))
    out = src + p
    assert p.dtype == out.dtype == np.float32
    return out


def perturb_observations(batch, alpha, *, obs_horizon, seed, draw, row_offset):
    """``noising.perturb_observations`` on a dict of numpy arrays (B, n, ...): cut to obs_horizon rows, then perturbed."""
    out = {}
    for i, k in enumerate(KEYS):
        cut = np.ascontiguousarray(batch[k][:, :obs_horizon], dtype=np.float32)
        out[k] = perturb(cut.reshape(len(cut), -1), alpha, seed=seed, draw=draw, purpose=4 + i, row_offset=row_offset).reshape(cut.shape)
    return out


def host_level(model, dataset, ids, *, runs, batch_size, seed, alpha, draw):
    """One noise level of ``evaluation.robustness`` the host way: the same chunks (restated here, not imported), the
    perturbation restated in numpy, ``model.sample`` on the uploaded observations, the errors of tests/eval_ref.py against the
    clean truth.  ``(position_error (N, P), action_error (N, P, 3))``."""
    import torch
    import eval_ref
    from state_policy_diffusionmodel_amd.evaluation import initial_noise
    obs_h, P, inp_h = model.obs_horizon, model.pred_horizon, model.inpaint_horizon
    N, st = len(ids) * runs, dataset.stats
    x_T = initial_noise(model, N, seed)
    pos, act = [], []
    for g0 in range(0, N, batch_size):
        g1 = min(N, g0 + batch_size)
        k0, k1 = g0 // runs, (g1 - 1) // runs + 1
        batch = dataset.batch(ids[k0:k1], frames="obs", with_translation=True)
        clean = {k: batch[k].cpu().numpy() for k in KEYS}
        noisy = perturb_observations(clean, alpha, obs_horizon=obs_h, seed=seed, draw=draw, row_offset=k0)
        obs = model.prepare_observation_batch({k: torch.from_numpy(v).to(model.device) for k, v in noisy.items()})
        cond, inpaint = model.prepare_obs_cond_vectors(obs), model.prepare_inpaint_vectors(obs)
        slot = eval_ref.slots(g0, g1 - g0, runs, k0)
        sel = torch.from_numpy(slot).to(model.device)
        x_0 = model.sample({"obs_cond": cond[sel], "inpaint": inpaint[sel]}, batched=True, sharded=False, x_T=x_T[g0:g1], seed=seed,
                           sample_offset=g0).cpu().numpy()[:, 0]
        tr = batch["translation"].cpu().numpy()
        pos.append(eval_ref.position_errors(x_0, clean["position"], tr, slot, float(st["position"]["min"]), float(st["position"]["max"]),
                                            obs_h, inp_h, P))
        act.append(eval_ref.action_errors(x_0, clean["action"], slot, st["action"]["min"], st["action"]["max"], obs_h, inp_h, P))
    return np.concatenate(pos), np.concatenate(act)
