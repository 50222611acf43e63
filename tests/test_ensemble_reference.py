"""tests/ensemble_ref.py, the restatement the GPU tests compare spdm_policy_select with, against properties that follow from its
definition in include/spdm.h.  No GPU."""
import numpy as np
import pytest

import ensemble_ref as er

POS_MIN, POS_MAX = -37.25, 61.5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _candidates(E, K, H, D, seed):
    return np.random.default_rng(seed).uniform(-1.2, 1.2, (E, K, H, D)).astype(np.float32)


@pytest.mark.parametrize("inp_h,cols", [(0, 2), (1, 5), (3, 3)])
def test_the_distance_matrix_is_symmetric_bit_for_bit_with_a_zero_diagonal(inp_h, cols):
    x = _candidates(4, 7, 9, 5, [inp_h, cols])
    d = er.distances(x, inp_h, cols)
    assert d.dtype == np.float64 and d.shape == (4, 7, 7)
    assert np.array_equal(_bits(d), _bits(d.transpose(0, 2, 1)))
    assert (d[:, np.arange(7), np.arange(7)] == 0.0).all() and (d >= 0.0).all()
    # one entry by hand, scalar by scalar in the stated order
    s = np.float64(0.0)
    for r in range(inp_h, 9):
        for c in range(cols):
            t = np.float64(x[2, 1, r, c]) - np.float64(x[2, 5, r, c])
            s = s + t * t
    assert s.tobytes() == d[2, 1, 5].tobytes()
    # columns >= cols and rows < inp_h do not enter
    y = x.copy()
    y[:, :, :inp_h] += 1.0
    y[:, :, :, cols:] -= 1.0
    assert np.array_equal(_bits(er.distances(y, inp_h, cols)), _bits(d))


def test_two_candidates_always_tie_and_the_first_is_kept():
    x = _candidates(50, 2, 8, 5, 1)
    chosen, out, scores, _ = er.select(x, er.MEDOID, 1, 5)
    assert np.array_equal(_bits(scores[:, 0]), _bits(scores[:, 1])) and (scores[:, 0] > 0).all()
    assert chosen.dtype == np.int32 and (chosen == 0).all()
    assert np.array_equal(out, x[:, 0])
    one = er.select(x[:, :1], er.MEDOID, 1, 5)
    assert (one[0] == 0).all() and (one[2] == 0.0).all()                     # K = 1: the score is d(0, 0) = 0


def test_duplicated_candidates_tie_towards_the_lower_index():
    x = _candidates(6, 5, 8, 2, 2)
    x[:, 3] = x[:, 1]                                                        # candidates 1 and 3 are the same plan
    chosen, _, scores, _ = er.select(x, er.MEDOID, 0, 2)
    assert np.array_equal(_bits(scores[:, 1]), _bits(scores[:, 3]))
    assert not (chosen == 3).any()
    x[:] = x[:, :1]                                                          # all five the same: every score is 0, the choice is 0
    chosen, _, scores, _ = er.select(x, er.MEDOID, 0, 2)
    assert (scores == 0.0).all() and (chosen == 0).all()
    guess = _candidates(6, 1, 8, 2, 3)[:, 0]
    chosen, _, scores, _ = er.select(x, er.COHERENT, 0, 2, guess=guess, rows=8)
    assert (scores == scores[:, :1]).all() and (chosen == 0).all()


def test_a_nan_score_never_wins_and_all_nan_is_candidate_zero():
    nan = np.nan
    s = np.array([[nan, 3.0, 1.0, 1.0], [2.0, nan, nan, 5.0], [nan, nan, nan, nan], [nan, nan, 7.0, nan], [np.inf, nan, np.inf, 9e300],
                  [np.inf, np.inf, nan, np.inf], [0.0, -0.0, 0.0, nan]])
    assert er.choose(s).tolist() == [2, 0, 0, 2, 3, 0, 0]
    # through the scores: a NaN in the scored part of candidate 0 poisons every distance to it, hence every medoid score
    x = _candidates(2, 4, 8, 5, 4)
    x[0, 0, 5, 1] = nan
    chosen, _, scores, _ = er.select(x, er.MEDOID, 1, 2)
    assert np.isnan(scores[0]).all() and chosen[0] == 0 and np.isfinite(scores[1]).all()
    # ... but only its own coherent score
    guess = _candidates(2, 1, 8, 5, 5)[:, 0]
    chosen, _, scores, _ = er.select(x, er.COHERENT, 1, 2, guess=guess, rows=7)
    assert np.isnan(scores[0, 0]) and np.isfinite(scores[0, 1:]).all() and chosen[0] == 1 + int(np.argmin(scores[0, 1:]))
    x[0, 0, 5, 1] = 0.0
    x[0, 0, 5, 4] = nan                                                      # outside cols: not looked at
    assert np.isfinite(er.select(x, er.MEDOID, 1, 2)[2]).all()


def test_a_bimodal_set():
    """Ten candidates around +m (six of them) and -m (four), the modes far apart against their width."""
    rng = np.random.default_rng(6)
    E, K, H, D, inp_h = 5, 10, 9, 5, 1
    m = rng.uniform(0.3, 0.6, (E, 1, H, D))
    sign = np.array([1, -1, 1, 1, -1, 1, -1, 1, -1, 1], dtype=np.float64)     # 60 % at +m, interleaved
    x = (sign[None, :, None, None] * m + 0.02 * rng.standard_normal((E, K, H, D))).astype(np.float32)
    chosen, out, scores, _ = er.select(x, er.MEDOID, inp_h, 2)
    assert (sign[chosen] == 1).all()                                         # the medoid lies in the larger mode
    assert np.array_equal(out, x[np.arange(E), chosen])
    guess = (-m[:, 0] + 0.02 * rng.standard_normal((E, H, D))).astype(np.float32)
    chosen, _, scores, _ = er.select(x, er.COHERENT, inp_h, 2, guess=guess, rows=H - inp_h)
    assert (sign[chosen] == -1).all()                                        # coherence with a plan in the smaller mode keeps it
    assert (scores[:, sign == -1].max(axis=1) < scores[:, sign == 1].min(axis=1)).all()
    # rows = 1 looks at row inp_h only: a guess that agrees with candidate 7 there and with nobody elsewhere
    guess = np.full((E, H, D), 9.0, dtype=np.float32)
    guess[:, inp_h] = x[:, 7, inp_h]
    chosen, _, scores, _ = er.select(x, er.COHERENT, inp_h, 5, guess=guess, rows=1)
    assert (chosen == 7).all() and (scores[:, 7] == 0.0).all()
    changed = x.copy()
    changed[:, :, inp_h + 1:] += 3.0
    changed[:, :, :inp_h] -= 3.0
    assert np.array_equal(_bits(er.coherent_scores(changed, guess, inp_h, 1, 5)), _bits(scores))
    assert (er.select(x, er.COHERENT, inp_h, 5, guess=guess, rows=2)[2][:, 7] > 0).all()


def test_the_spread_of_identical_candidates_is_exactly_zero():
    """With K = 1 or 2 the mean of K equal values is that value exactly (u, and u + u halved).  For other K the running sum
    j u must not round, which holds where u has few mantissa bits: here U maps n = i / 8, translation 0, statistics [0, 2048] to
    the integer 256 (i + 4) below 2^12, so every sum of up to K = 64 terms is an integer below 2^18."""
    rng = np.random.default_rng(7)
    for K in (1, 2):
        x = np.repeat(_candidates(3, 1, 9, 5, [7, K]), K, axis=1)
        tr = rng.uniform(-1, 1, (3, 2)).astype(np.float32)
        assert (er.spread(x, tr, POS_MIN, POS_MAX, 1) == 0.0).all()
    for K in (3, 5, 64):
        one = (rng.integers(-8, 9, (3, 1, 9, 5)) / 8.0).astype(np.float32)
        sp = er.spread(np.repeat(one, K, axis=1), np.zeros((3, 2), np.float32), 0.0, 2048.0, 1)
        assert sp.shape == (3, 8) and (sp == 0.0).all()


def test_the_spread_of_two_candidates_is_half_their_distance():
    """K = 2: mu = (u_0 + u_1) / 2, both deviations are half the difference, and the root of the mean of two equal terms is
    that half.  Each of u_0 + u_1, u_k - mu rounds once at the magnitude of u, the rest is relative: 4 ulp of max |u| covers it."""
    rng = np.random.default_rng(8)
    E, H, inp_h = 40, 9, 1
    x = _candidates(E, 2, H, 5, 8)
    tr = rng.uniform(-1, 1, (E, 2)).astype(np.float32)
    sp = er.spread(x, tr, POS_MIN, POS_MAX, inp_h)
    u = er.U(x[:, :, inp_h:, 0], tr[:, None, None, 0], POS_MIN, POS_MAX)
    v = er.U(x[:, :, inp_h:, 1], tr[:, None, None, 1], POS_MIN, POS_MAX)
    d = np.hypot(u[:, 0] - u[:, 1], v[:, 0] - v[:, 1])
    bound = 4 * np.finfo(np.float64).eps * max(np.abs(u).max(), np.abs(v).max())
    assert sp.shape == (E, H - inp_h) and (d > 1.0).any()
    assert np.abs(sp - d / 2).max() <= bound
    # in the dataset's units: the statistics' range scales it, the translation moves both candidates alike
    twice = er.spread(x, tr, 2 * POS_MIN, 2 * POS_MAX, inp_h)
    assert np.allclose(twice, 2 * sp, rtol=1e-12, atol=0)
    moved = er.spread(x, (tr + np.float32(0.25)).astype(np.float32), POS_MIN, POS_MAX, inp_h)
    assert np.abs(moved - sp).max() <= 2 * (bound + 4 * np.finfo(np.float64).eps * 0.125 * (POS_MAX - POS_MIN))


def test_select_returns_the_chosen_row_unchanged():
    x = _candidates(7, 5, 8, 5, 9)
    tr = np.zeros((7, 2), np.float32)
    chosen, out, scores, sp = er.select(x, er.MEDOID, 0, 5, translation=tr, pos_min=POS_MIN, pos_max=POS_MAX)
    assert out.dtype == np.float32 and out.shape == (7, 8, 5) and sp.shape == (7, 8) and scores.shape == (7, 5)
    for e in range(7):
        assert np.array_equal(out[e], x[e, chosen[e]]) and scores[e, chosen[e]] == scores[e].min()
    assert len(set(chosen.tolist())) > 1
