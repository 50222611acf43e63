"""tests/loss_terms_ref.py (the restatement of spdm_loss_terms' summation order) against numpy's own mean: a reordered
float64 sum of n non-negative terms differs from any other order by at most n 2^-53 relative."""
import numpy as np
import pytest

import loss_terms_ref

U = 2.0 ** -53


@pytest.mark.parametrize("B,H,D", [(1, 8, 1), (3, 31, 5), (2, 32, 3), (5, 64, 6), (4, 1, 1), (2, 64, 1), (2, 13, 5)])
def test_terms_agree_with_numpy_mean(B, H, D):
    rng = np.random.default_rng([B, H, D])
    eps = rng.standard_normal((B, H, D)).astype(np.float32)
    noise = rng.standard_normal((B, H, D)).astype(np.float32)
    got = loss_terms_ref.loss_terms(eps, noise)
    assert got.shape == (B,) and got.dtype == np.float64
    for b in range(B):
        want = np.mean((noise[b].astype(np.float64) - eps[b].astype(np.float64)) ** 2)
        rel = abs(got[b] - want) / want
        print(f"(B,H,D) = ({B},{H},{D}) sample {b}: rel diff {rel:.3e}, bound {H * D * U:.3e}")
        assert rel <= H * D * U


def test_an_explicit_small_case():
    """n = 3: partials 0..2 hold one square each; the tree gives (p0 + p2) + p1 (offsets 2 then 1), every other add is + 0.0."""
    eps = np.array([[0.5, -1.25, 3.0]], dtype=np.float32)
    noise = np.array([[1.5, 0.25, -1.0]], dtype=np.float32)
    sq = (noise.astype(np.float64) - eps.astype(np.float64)) ** 2
    want = ((sq[0, 0] + sq[0, 2]) + sq[0, 1]) / 3.0
    assert loss_terms_ref.loss_terms(eps, noise)[0] == want


def test_the_order_is_not_numpys_for_a_long_row():
    """Several elements per partial: the restatement is a specific order, not np.sum's -- some seed shows a last-bit difference."""
    differs = 0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        eps = rng.standard_normal((1, 64, 6)).astype(np.float32)
        noise = rng.standard_normal((1, 64, 6)).astype(np.float32)
        seq = np.float64(0.0)
        for v in ((noise.astype(np.float64) - eps.astype(np.float64)) ** 2).reshape(-1):
            seq = seq + v
        differs += loss_terms_ref.loss_terms(eps, noise)[0] != seq / 384.0
    assert differs > 0


def test_identical_inputs_give_zero_and_a_split_batch_changes_nothing():
    rng = np.random.default_rng(3)
    eps = rng.standard_normal((5, 31, 5)).astype(np.float32)
    noise = rng.standard_normal((5, 31, 5)).astype(np.float32)
    assert not loss_terms_ref.loss_terms(eps, eps).any()
    whole = loss_terms_ref.loss_terms(eps, noise)
    parts = np.concatenate([loss_terms_ref.loss_terms(eps[:3], noise[:3]), loss_terms_ref.loss_terms(eps[3:], noise[3:])])
    assert np.array_equal(whole, parts)


@pytest.mark.parametrize("N", [1, 12, 64, 300, 1024, 1025, 3000])
def test_pass_mean_agrees_with_numpy_mean(N):
    terms = np.abs(np.random.default_rng(N).standard_normal(N)) + 0.1
    got, want = loss_terms_ref.pass_mean(terms), np.mean(terms)
    assert abs(got - want) / want <= N * U
