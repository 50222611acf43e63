"""MaxPool2d(2) of a tensor whose GroupNorm is still pending, taken on the RAW values (csrc/conv_reg.hip's pooled epilogue,
DESIGN.md 4.2): a float32 restatement of pool_kernel's arithmetic, no GPU.

pool_kernel (csrc/elementwise.hip) finishes each of the four values of a window with affine1 (csrc/resample.h),

    affine1(v) = fma(sc, v - mu, be),   sc = rstd * gamma,  rstd > 0,

and takes max(max(a00, a01), max(a10, a11)).  Both operations of affine1 are correctly rounded, hence monotone in v:
non-decreasing for sc >= 0, non-increasing for sc < 0.  So the max of the finished values is affine1 of the raw max where
gamma >= 0 and affine1 of the raw min where gamma < 0 -- bit for bit, which is what lets the producer store one raw value per
window and the consumer apply the affine once.  The one exception: sc == +-0 (gamma zero, or tiny enough that rstd * gamma
underflows) with be == 0, where every finished value is a zero whose sign follows the sign of v - mu.
"""
import numpy as np
import pytest

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """float32 fma(a, b, c), one rounding: the product of two float32 is exact in float64; the sum is rounded to odd in float64
    (TwoSum gives the residual), which the final rounding to float32 turns into the correctly rounded result."""
    p = a.astype(F64) * b.astype(F64)
    c = np.broadcast_to(c, p.shape).astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    with np.errstate(over="ignore", under="ignore"):
        return np.where((err != 0) & even, odd, s).astype(F32)


def affine1(v, mu, sc, be):
    return fma32(np.broadcast_to(sc, v.shape).astype(F32), (v - mu).astype(F32), be)


def max4(x):
    """pool_kernel's order; x: (..., 4) = v00, v01, v10, v11"""
    return np.maximum(np.maximum(x[..., 0], x[..., 1]), np.maximum(x[..., 2], x[..., 3]))


def min4(x):
    return np.minimum(np.minimum(x[..., 0], x[..., 1]), np.minimum(x[..., 2], x[..., 3]))


def pool_finished(v, mu, sc, be):
    """what pool_kernel computes: the affine per tap, then the max"""
    return max4(affine1(v, mu, sc[:, None], be[:, None]))


def pool_raw_then_affine(v, mu, gamma, sc, be, always_max=False):
    """the producer's epilogue (select on the sign of the gain) followed by the consumer's prologue"""
    sel = max4(v) if always_max else np.where(gamma >= 0, max4(v), min4(v))
    return affine1(sel.astype(F32), mu, sc, be)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.int32)


def windows(kind, n, seed):
    """(n, 4) raw values; mean, rstd; per-window gain and offset"""
    g = np.random.default_rng(seed)
    v = (g.standard_normal((n, 4)) * g.choice([1e-3, 1.0, 40.0], (n, 1))).astype(F32)
    if kind == "ties":
        v[:, 1] = v[:, 0]
        v[::2, 3] = v[::2, 2]
        v[::3, 2] = v[::3, 0]
    elif kind == "zeros":
        v[:, 0] = 0.0
        v[::2, 1] = -0.0
        v[::3, 2] = -0.0
        v[::5] = np.array([0.0, -0.0, -0.0, 0.0], dtype=F32)
    elif kind == "close":
        # neighbours one ulp apart: v - mu and the fma round them onto equal or adjacent results
        v[:, 1] = np.nextafter(v[:, 0], F32(np.inf))
        v[:, 2] = np.nextafter(v[:, 0], F32(-np.inf))
        v[:, 3] = np.nextafter(v[:, 1], F32(np.inf))
    mu = F32(g.standard_normal() * 0.3 + 0.11)
    rstd = F32(abs(g.standard_normal()) + 0.25)
    gamma = (g.standard_normal(n) * g.choice([1e-4, 1.0, 3.0], n)).astype(F32)
    be = (g.standard_normal(n) + 0.01).astype(F32)
    be[be == 0] = F32(0.5)
    return v, mu, rstd, gamma, be


@pytest.mark.parametrize("kind", ["random", "ties", "zeros", "close"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_max_of_finished_equals_affine_of_selected_raw(kind, seed):
    v, mu, rstd, gamma, be = windows(kind, 20000, seed)
    assert (gamma < 0).sum() > 1000 and (gamma > 0).sum() > 1000
    sc = (rstd * gamma).astype(F32)
    want = pool_finished(v, mu, sc, be)
    got = pool_raw_then_affine(v, mu, gamma, sc, be)
    assert np.array_equal(bits(want), bits(got)), int((bits(want) != bits(got)).sum())


def test_zero_and_underflowing_gains():
    """gamma = +-0 and gains whose product with rstd underflows to +-0: every finished value is be, whichever raw value was
    selected (be != 0 here)."""
    v, mu, rstd, gamma, be = windows("random", 4096, 7)
    rstd = F32(0.5)
    tiny = F32(1.4e-45)                       # the smallest denormal: 0.5 * tiny rounds to zero
    gamma[0::4] = 0.0
    gamma[1::4] = -0.0
    gamma[2::4] = tiny
    gamma[3::4] = -tiny
    sc = (rstd * gamma).astype(F32)
    assert np.all(sc == 0)
    want = pool_finished(v, mu, sc, be)
    got = pool_raw_then_affine(v, mu, gamma, sc, be)
    assert np.array_equal(bits(want), bits(be))
    assert np.array_equal(bits(want), bits(got))


def test_zero_gain_and_zero_offset_is_a_zero_of_either_sign():
    """The documented exception: sc == +-0 and be == 0.  Both sides are zeros; only the sign may differ."""
    v, mu, rstd, gamma, be = windows("random", 4096, 9)
    gamma[0::2] = 0.0
    gamma[1::2] = -0.0
    be[:] = 0.0
    be[: be.size // 2] = -0.0                        # (+-0) + (+0) is +0 whatever the product's sign; only be = -0 keeps it
    sc = (rstd * gamma).astype(F32)
    want = pool_finished(v, mu, sc, be)
    got = pool_raw_then_affine(v, mu, gamma, sc, be)
    assert np.all(want == 0) and np.all(got == 0)
    half = be.size // 2
    assert np.array_equal(bits(want[half:]), bits(got[half:])) and np.all(bits(got[half:]) == 0)
    assert (bits(want[:half]) != bits(got[:half])).any()           # (the case is real: the bits do differ somewhere)


def test_always_max_mutant_fails_on_negative_gains():
    v, mu, rstd, gamma, be = windows("random", 20000, 3)
    gamma = -np.abs(gamma) - F32(0.05)
    sc = (rstd * gamma).astype(F32)
    want = pool_finished(v, mu, sc, be)
    mutant = pool_raw_then_affine(v, mu, gamma, sc, be, always_max=True)
    assert (bits(want) != bits(mutant)).mean() > 0.9
    assert np.array_equal(bits(want), bits(pool_raw_then_affine(v, mu, gamma, sc, be)))


def test_fma32_is_one_rounding():
    """the helper itself: cases where float64 arithmetic rounded twice differs from a fused multiply-add"""
    a = np.array([1.0 + 2.0 ** -23, 3.0, 1.0 + 2.0 ** -12], dtype=F32)
    b = np.array([1.0 + 2.0 ** -23, 1.0 / 3.0, 1.0 + 2.0 ** -12], dtype=F32)
    c = np.array([-1.0, -1.0, 2.0 ** -30], dtype=F32)
    from fractions import Fraction
    for i in range(3):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        got = Fraction(float(fma32(a[i:i + 1], b[i:i + 1], c[i:i + 1])[0]))
        lo, hi = np.nextafter(F32(float(got)), F32(-np.inf)), np.nextafter(F32(float(got)), F32(np.inf))
        assert abs(exact - got) <= abs(exact - Fraction(float(lo))) and abs(exact - got) <= abs(exact - Fraction(float(hi)))
