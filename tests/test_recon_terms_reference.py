"""tests/recon_terms_ref.py (the restatement of spdm_recon_terms' summation order) against torch's own per-frame float64 mean:
a reordered sum agrees with it to the rounding bound, and every way of getting the order or the arithmetic wrong that the
restatement could hide shows on this data."""
import numpy as np
import pytest
import torch

import recon_terms_ref

FRAME = recon_terms_ref.FRAME
U = 2.0 ** -53


def _pairs(n=5, seed=11):
    """reconstructions near 0.5 (an untrained decoder's), targets over [0, 1), and errors of mixed magnitude in one frame"""
    rng = np.random.default_rng(seed)
    target = rng.random((n, 3, 96, 96), dtype=np.float32)
    recon = (0.5 + 0.05 * rng.standard_normal((n, 3, 96, 96))).astype(np.float32)
    flat = recon[-1].reshape(-1)
    flat[:] = target[-1].reshape(-1)
    flat[0::2] += np.float32(1e-4)
    flat[1::2] -= np.float32(1.0)
    return recon, target


def test_restatement_agrees_with_torchs_float64_mean():
    """Both are sums of 27648 non-negative float64 squares, the same squares, in different orders.  A sum of non-negative
    terms in ANY order is within (additions on the longest path) x 2^-53 of the exact sum, relatively: at most 27647 for
    torch, whose order is not known, and 27 x 4 + 8 = 116 for the restatement; each division adds one rounding.  So the two
    differ by at most (27647 + 116 + 2) x 2^-53 = 3.1e-12 relative."""
    recon, target = _pairs()
    got = recon_terms_ref.recon_terms(recon, target)
    want = torch.mean((torch.from_numpy(target).double() - torch.from_numpy(recon).double()) ** 2, dim=(1, 2, 3)).numpy()
    rel = np.abs(got - want) / want
    bound = (FRAME - 1 + 116 + 2) * U
    print(f"max rel diff {rel.max():.3e} (bound {bound:.3e})")
    assert got.dtype == np.float64 and got.shape == (5,)
    assert (rel <= bound).all()


def test_identical_frames_give_exact_zero_and_frames_are_independent():
    recon, target = _pairs()
    assert not recon_terms_ref.recon_terms(target, target).any()
    whole = recon_terms_ref.recon_terms(recon, target)
    parts = np.concatenate([recon_terms_ref.recon_terms(recon[:2], target[:2]), recon_terms_ref.recon_terms(recon[2:], target[2:])])
    assert np.array_equal(whole.view(np.uint64), parts.view(np.uint64))


def test_a_single_error_lands_whole_wherever_it_is():
    for e in (0, 3, 4, 1023, 1024, FRAME - 4, FRAME - 1):
        target = np.zeros((1, 3, 96, 96), np.float32)
        recon = target.copy()
        recon.reshape(-1)[e] = 0.5
        assert recon_terms_ref.recon_terms(recon, target)[0] == 0.25 / FRAME, e


@pytest.mark.parametrize("name,knobs", [("float32 accumulation", {"acc": np.float32}), ("divisor n x 27648", {"divisor": 5 * FRAME}),
                                         ("last quad dropped", {"drop_last_quad": True}), ("t + r", {"sign": 1.0}),
                                         ("partial = q mod 64", {"partials": 64})])
def test_mutants_of_the_restatement_show(name, knobs):
    recon, target = _pairs()
    true = recon_terms_ref.recon_terms(recon, target)
    mutant = recon_terms_ref.recon_terms(recon, target, **knobs)
    assert not np.array_equal(true.view(np.uint64), mutant.view(np.uint64)), name
