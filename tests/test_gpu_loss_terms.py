"""spdm_loss_terms (csrc/train_metrics.hip) against its numpy restatement tests/loss_terms_ref.py bit for bit, and
spdm_unet_forward_dt against spdm_unet_forward bit for bit.  The terms are chains of correctly rounded float64 operations in a
fixed order, so their tolerance is zero."""
import math

import numpy as np
import pytest
import torch

import loss_terms_ref

pytestmark = pytest.mark.gpu

CASES = [(1, 8, 1), (3, 31, 5), (2, 32, 3), (5, 64, 6)]      # H x D = 8 (below a wave), 155 and 96 (no multiple of 64), 384 (6 rows per lane)
SENTINEL, T_SENTINEL = -7.0, -9


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, got.dtype, want.shape, want.dtype)
    diff = np.count_nonzero(got.view(np.uint64) != want.view(np.uint64))
    assert diff == 0, f"{what}: {diff} of {got.size} elements differ"


def _inputs(B, H, D, seed=0):
    rng = np.random.default_rng([B, H, D, seed])
    eps = rng.standard_normal((B, H, D)).astype(np.float32)
    noise = rng.standard_normal((B, H, D)).astype(np.float32)
    t = rng.integers(0, 1000, B).astype(np.int32)
    return eps, noise, t


@pytest.mark.parametrize("with_t", [False, True])
@pytest.mark.parametrize("slot_offset", [0, 2])
@pytest.mark.parametrize("B,H,D", CASES)
def test_terms_equal_the_restatement_bit_for_bit(B, H, D, slot_offset, with_t):
    from state_policy_diffusionmodel_amd.train_metrics import loss_terms_into
    eps, noise, t = _inputs(B, H, D)
    n_slots = slot_offset + B + 3
    terms = torch.full((n_slots,), SENTINEL, dtype=torch.float64, device="cuda")
    slot_t = torch.full((n_slots,), T_SENTINEL, dtype=torch.int32, device="cuda")
    shape = (B, 1, H, D) if with_t else (B, H, D)            # both layouts the wrapper takes
    loss_terms_into(torch.from_numpy(eps).cuda().view(shape), torch.from_numpy(noise).cuda().view(shape), terms, slot_offset,
                    t=torch.from_numpy(t).cuda() if with_t else None, slot_t=slot_t if with_t else None)
    got, got_t = terms.cpu().numpy(), slot_t.cpu().numpy()
    want = loss_terms_ref.loss_terms(eps, noise)
    assert np.isfinite(want).all() and want.min() > 0
    same_bits(got[slot_offset:slot_offset + B], want, (B, H, D, slot_offset))
    assert (got[:slot_offset] == SENTINEL).all() and (got[slot_offset + B:] == SENTINEL).all()      # untouched on both sides
    if with_t:
        assert np.array_equal(got_t[slot_offset:slot_offset + B], t)
        assert (got_t[:slot_offset] == T_SENTINEL).all() and (got_t[slot_offset + B:] == T_SENTINEL).all()
    else:
        assert (got_t == T_SENTINEL).all()


def test_a_batch_in_two_calls_equals_one_call():
    from state_policy_diffusionmodel_amd.train_metrics import loss_terms_into
    eps, noise, t = _inputs(5, 64, 6, seed=1)
    d_eps, d_noise, d_t = (torch.from_numpy(a).cuda() for a in (eps, noise, t))
    one, one_t = torch.empty(5, dtype=torch.float64, device="cuda"), torch.empty(5, dtype=torch.int32, device="cuda")
    loss_terms_into(d_eps, d_noise, one, 0, t=d_t, slot_t=one_t)
    two, two_t = torch.full((5,), SENTINEL, dtype=torch.float64, device="cuda"), torch.full((5,), T_SENTINEL, dtype=torch.int32, device="cuda")
    loss_terms_into(d_eps[:3], d_noise[:3], two, 0, t=d_t[:3], slot_t=two_t)
    assert (two[3:] == SENTINEL).all() and (two_t[3:] == T_SENTINEL).all()
    loss_terms_into(d_eps[3:], d_noise[3:], two, 3, t=d_t[3:], slot_t=two_t)
    same_bits(two.cpu().numpy(), one.cpu().numpy(), "two calls")
    same_bits(one.cpu().numpy(), loss_terms_ref.loss_terms(eps, noise), "one call")
    assert torch.equal(one_t, two_t) and np.array_equal(one_t.cpu().numpy(), t)


@pytest.mark.parametrize("B,H,D", [(5, 64, 6), (37, 31, 5), (1300, 8, 1)])     # 1300 terms: two blocks of the reduction
def test_the_reduced_mean_against_torchs_fp32_mean(B, H, D):
    """spdm_eval_reduce over the (B, 1) terms: val_loss.  Bit for bit the restated order; within 1e-5 relative of torch's fp32
    mean((noise - eps)^2) over the same elements (fp32 pairwise summation errs by about log2(n) 2^-24 ~ 1.3e-6 for n <= 2^20,
    with a few times' margin)."""
    from state_policy_diffusionmodel_amd.evaluation import reduce_errors
    from state_policy_diffusionmodel_amd.train_metrics import loss_terms_into
    eps, noise, _ = _inputs(B, H, D, seed=2)
    d_eps, d_noise = torch.from_numpy(eps).cuda(), torch.from_numpy(noise).cuda()
    terms = torch.empty(B, dtype=torch.float64, device="cuda")
    loss_terms_into(d_eps, d_noise, terms)
    wmean, wstd, mean, std = reduce_errors(terms.view(B, 1), 1)
    got = float(mean.item())
    same_bits(np.array([got]), np.array([loss_terms_ref.pass_mean(loss_terms_ref.loss_terms(eps, noise))]), "pass mean")
    assert torch.equal(wmean.view(-1), terms) and not wstd.any()              # runs = 1: a window is one term
    want = float(torch.mean((d_noise - d_eps) ** 2).item())
    exact = math.fsum(((noise.astype(np.float64) - eps.astype(np.float64)) ** 2).reshape(-1).tolist()) / (B * H * D)
    print(f"(B,H,D) = ({B},{H},{D}): device {got!r}, torch fp32 {want!r}, rel diff {abs(got - want) / want:.3e} (bound 1e-5); "
          f"vs exact {abs(got - exact) / exact:.3e}")
    assert abs(got - want) <= 1e-5 * want
    assert abs(got - exact) <= (B + H * D + 4) * 2.0 ** -53 * exact       # both sums in any order, the squares, the two divisions


@pytest.mark.parametrize("model", ["UNet_FilmnoAttention", "UNet"])
def test_unet_forward_dt_equals_unet_forward_bit_for_bit(model):
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    from state_policy_diffusionmodel_amd.weights import random_state_dict
    B, H, D, cond_dim, T = 2, 16, 3, 14, 30
    rows = T + 1 if model == "UNet" else T                   # simple_Unet.py's table has noise_steps + 1 rows
    eng = SpdmEngine(H, D, cond_dim, max_batch=B, num_train_timesteps=rows, model=model)
    eng.load_state_dict(random_state_dict(cond_dim, seed=3, attention=False, model=model, noise_steps=T))
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 1, H, D, generator=g).cuda()
    cond = torch.randn(B, 1, 2, 7, generator=g).cuda()
    try:
        for t in ([0, rows - 1], [rows - 1, 0], [7]):        # per-sample t with both ends of the table; one t for the batch
            host = eng.unet_forward(x, torch.tensor(t, dtype=torch.int64), cond)
            dev = eng.unet_forward(x, torch.tensor(t, dtype=torch.int32).cuda(), cond)
            assert torch.isfinite(host).all() and host.abs().max() > 0
            assert torch.equal(host, dev), t
        # outside [0, T): clamped by the copy kernel, no table is read out of range
        clamped = eng.unet_forward(x, torch.tensor([-5, rows + 100], dtype=torch.int32).cuda(), cond)
        assert torch.equal(clamped, eng.unet_forward(x, torch.tensor([0, rows - 1], dtype=torch.int64), cond))
        with pytest.raises(RuntimeError, match="outside"):   # the host entry still refuses
            eng.unet_forward(x, torch.tensor([0, rows], dtype=torch.int64), cond)
    finally:
        eng.close()
