"""tests/warm_start_ref.py, the restatement the GPU tests compare spdm_policy_warm_start with, against independent float64
arithmetic on the same float32 inputs, and the properties include/spdm.h states.  No GPU.

Bounds (u = 2^-24, the unit roundoff of float32; M = max(|a|, |b|)):
  interpolation g = a + w (b - a): w carries u, b - a (at most 2M) carries u, the product (at most 2M) u again, and the sum, which
    lies between a and b, u M: at most about 7 u M < 2^-21 M.  Measured on 2 10^5 cases for each of seven (f, step_size): 0.54 of the bound.
  re-centring g' = ((2g + T0) - T1) / 2 with sn = 2g + T0: the sum carries u |sn|, the difference u |sn - T1| (1 + u), the
    scalings are exact: |g' - exact| <= (u |sn| + u |sn - T1|) / 2 (1 + u) < 2^-23 max(|sn|, |sn - T1|).  Measured: 0.49 of the bound."""
import numpy as np
import pytest

import policy_ref
import warm_start_ref as ws

N_CASES = 200_000


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _plan(rng, E, H, D):
    return rng.uniform(-1.2, 1.2, (E, H, D)).astype(np.float32)


def test_interpolation_stays_within_its_bound_of_float64():
    rng = np.random.default_rng(1)
    scale = np.exp2(rng.integers(-20, 21, N_CASES)).astype(np.float32)
    a = (rng.standard_normal(N_CASES).astype(np.float32) * scale)
    b = (rng.standard_normal(N_CASES).astype(np.float32) * scale * np.exp2(rng.integers(-3, 4, N_CASES)).astype(np.float32))
    worst = 0.0
    for step_size, f in ((2, 1), (3, 1), (3, 2), (5, 3), (7, 6), (50, 49), (1000, 1)):
        prev = np.ascontiguousarray(np.stack([a, b], axis=1)[:, :, None].repeat(2, axis=2))       # E = N_CASES, H = 2, D = 2
        g = ws.shift(prev, f, step_size)[:, 0, 0]                            # row 0 lies between rows 0 and 1
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        exact = a64 + (f / step_size) * (b64 - a64)
        bound = np.exp2(-21) * np.maximum(np.abs(a64), np.abs(b64))
        err = np.abs(g.astype(np.float64) - exact)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (step_size, f, float((err / bound).max()))
    print(f"interpolation: worst error {worst:.3f} of the bound")


def test_recentring_stays_within_its_bound_of_float64():
    rng = np.random.default_rng(2)
    g = rng.uniform(-1.5, 1.5, (N_CASES, 1, 2)).astype(np.float32)
    T0 = rng.uniform(-2.0, 2.0, (N_CASES, 2)).astype(np.float32)
    T1 = (T0 + rng.standard_normal((N_CASES, 2)).astype(np.float32) * np.exp2(rng.integers(-12, 1, (N_CASES, 1))).astype(np.float32))
    got = ws.recentre(g, T0, T1).astype(np.float64)
    sn = 2.0 * g.astype(np.float64) + T0.astype(np.float64)[:, None, :]
    exact = (sn - T1.astype(np.float64)[:, None, :]) / 2.0
    bound = np.exp2(-23) * np.maximum(np.abs(sn), np.abs(sn - T1.astype(np.float64)[:, None, :]))
    err = np.abs(got - exact)
    print(f"re-centring: worst error {float((err / bound).max()):.3f} of the bound")
    assert (err <= bound).all()


def test_no_shift_and_no_translation_change_return_the_previous_plan():
    """delta = 0 and T0 == T1.  The action columns come back bit for bit whatever the values.  The position columns go through
    ((2g + T0) - T0) / 2, whose first sum rounds: they come back bit for bit wherever 2g + T0 is a float32 (checked on a
    2^-12 grid, and with T0 = 0), and within the re-centring bound otherwise."""
    rng = np.random.default_rng(3)
    prev = _plan(rng, 4, 16, 5)
    T = rng.uniform(-1.0, 1.0, (4, 2)).astype(np.float32)
    g = ws.guess(prev, T, T, 0, 3)
    assert np.array_equal(_bits(g[:, :, 2:]), _bits(prev[:, :, 2:]))
    sn = 2.0 * prev[:, :, :2].astype(np.float64) + T.astype(np.float64)[:, None, :]
    bound = np.exp2(-23) * np.maximum(np.abs(sn), np.abs(sn - T.astype(np.float64)[:, None, :]))
    assert (np.abs(g[:, :, :2].astype(np.float64) - prev[:, :, :2].astype(np.float64)) <= bound).all()
    zero = np.zeros((4, 2), np.float32)
    assert np.array_equal(_bits(ws.guess(prev, zero, zero, 0, 3)), _bits(prev))
    grid = (rng.integers(-4096, 4097, (4, 16, 5)) / 4096.0).astype(np.float32)
    Tg = (rng.integers(-8192, 8193, (4, 2)) / 4096.0).astype(np.float32)
    assert np.array_equal(_bits(ws.guess(grid, Tg, Tg, 0, 3)), _bits(grid))


def test_a_whole_shift_does_no_interpolation_arithmetic():
    """f == 0: -0.0, subnormals, infinities and NaN payloads pass through the action columns unchanged."""
    rng = np.random.default_rng(4)
    prev = _plan(rng, 2, 8, 5)
    odd = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00123], dtype=np.uint32).view(np.float32)
    prev[0, 1:7, 2] = odd
    prev[1, 2:8, 4] = odd
    T0, T1 = rng.uniform(-1, 1, (2, 2)).astype(np.float32), rng.uniform(-1, 1, (2, 2)).astype(np.float32)
    for delta, q in ((0, 0), (3, 1), (6, 2), (21, 7)):
        g = ws.guess(prev, T0, T1, delta, 3)
        want = prev[:, np.minimum(np.arange(8) + q, 7), :]
        assert np.array_equal(_bits(g[:, :, 2:]), _bits(want[:, :, 2:])), delta


@pytest.mark.parametrize("delta", [44, 45, 46, 1000, 10 ** 12])
def test_rows_past_the_end_hold_the_last_row(delta):
    rng = np.random.default_rng(5)
    H, s = 16, 3
    prev = _plan(rng, 3, H, 5)
    T0, T1 = rng.uniform(-1, 1, (3, 2)).astype(np.float32), rng.uniform(-1, 1, (3, 2)).astype(np.float32)
    g = ws.guess(prev, T0, T1, delta, s)
    q, f = divmod(delta, s)
    first_held = max(0, H - 1 - q)                                           # r + q >= H - 1
    last = ws.recentre(prev[:, H - 1:, :], T0, T1)
    held = g[:, first_held:, :].astype(np.float64)
    assert first_held < H
    # a + w (a - a) = a + 0 is a again (these values hold no -0.0)
    assert np.array_equal(held, np.broadcast_to(last.astype(np.float64), held.shape))
    if first_held > 0:
        assert not np.array_equal(g[:, first_held - 1, :], g[:, first_held, :])


@pytest.mark.parametrize("delta", [0, 3, 9, 42])
def test_whole_shifts_keep_the_waypoints_where_they_were(delta):
    """U(guess, T1) equals U(old plan at the shifted rows, T0) within the float64 image of the re-centring bound: with
    n' = g' the error of 2 n' + T1 against 2 n + T0 is twice the bound, U scales it by (max - min) / 2; U's own float64
    operations (five, on values no larger than |min| + (max - min) (1 + |s|)) add a few 2^-53 of that."""
    rng = np.random.default_rng(6)
    E, H, s, inp_h = 3, 16, 3, 1
    lo, hi = -312.5, 977.25
    prev = _plan(rng, E, H, 5)
    T0 = rng.uniform(-1, 1, (E, 2)).astype(np.float32)
    T1 = (T0 + rng.uniform(-0.05, 0.05, (E, 2))).astype(np.float32)
    g = ws.guess(prev, T0, T1, delta, s)
    shifted = prev[:, np.minimum(np.arange(H) + delta // s, H - 1), :]
    got = policy_ref.U(np.ascontiguousarray(g[:, inp_h:, :2]), T1, lo, hi)
    want = policy_ref.U(np.ascontiguousarray(shifted[:, inp_h:, :2]), T0, lo, hi)
    sn = 2.0 * shifted[:, inp_h:, :2].astype(np.float64) + T0.astype(np.float64)[:, None, :]
    bound = np.exp2(-23) * np.maximum(np.abs(sn), np.abs(sn - T1.astype(np.float64)[:, None, :])) * (hi - lo)
    bound = bound + 16 * np.exp2(-53) * (abs(lo) + (hi - lo) * (1.0 + np.abs(sn)))
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / bound).max())


def test_only_the_inpainted_rows_of_x_are_the_inpaint_vector():
    rng = np.random.default_rng(7)
    E, H, D, inp_h = 3, 9, 5, 4
    prev, inpaint = _plan(rng, E, H, D), _plan(rng, E, inp_h, D)
    T0, T1 = rng.uniform(-1, 1, (E, 2)).astype(np.float32), rng.uniform(-1, 1, (E, 2)).astype(np.float32)
    sa, sb = np.float32(0.8306), np.float32(0.5568)
    x, g, z = ws.warm_start(prev, T0, T1, inpaint, 7, 5, sa, sb, seed=11, env_offset=2, draw_index=3)
    assert x.dtype == g.dtype == z.dtype == np.float32 and x.shape == g.shape == z.shape == (E, H, D)
    free = sa * g + sb * z
    assert np.array_equal(_bits(x[:, :inp_h]), _bits(inpaint))
    assert np.array_equal(_bits(x[:, inp_h:]), _bits(free[:, inp_h:]))
    assert not np.array_equal(free[:, :inp_h], inpaint)                      # guess and noise are not in-painted
    assert np.array_equal(_bits(g), _bits(ws.guess(prev, T0, T1, 7, 5)))
    x2, _, z2 = ws.warm_start(prev, T0, T1, None, 7, 5, sa, sb, noise=z)
    assert z2 is z and np.array_equal(_bits(x2), _bits(free))


def test_the_noise_is_its_own_stream_and_shards_like_the_whole():
    import forward_process_ref
    E, H, D = 4, 9, 5
    z = ws.draw(11, 3, 0, E, H, D)
    assert np.isfinite(z).all() and abs(float(z.mean())) < 0.3 and 0.7 < float(z.std()) < 1.3
    assert np.array_equal(ws.draw(11, 3, 2, 2, H, D), z[2:])                 # a shard draws what the whole would
    assert np.array_equal(ws.draw(11, 3, 2 ** 32, E, H, D), z)               # the global index is taken mod 2^32
    for other in (ws.draw(12, 3, 0, E, H, D), ws.draw(11, 4, 0, E, H, D), ws.draw(11 + 2 ** 32, 3, 0, E, H, D)):
        assert not np.array_equal(other, z)
    assert not np.array_equal(z[0], z[1])
    for purpose in (1, 2, 3, 4, 5, 6, 7):
        assert not np.array_equal(forward_process_ref.draw_noise(11, 3, 0, E, H * D, purpose=purpose).reshape(E, H, D), z)
