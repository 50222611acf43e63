#!/usr/bin/env python3
"""Coefficients of the one-exponential GELU of csrc/device_utils.h (gelu_erf), and its float32-emulated error.  No GPU needed.

    gelu(v) = max(v, 0) - x q(x),   x = min(|v|, 6),   q(x) = Phi(-x) = 0.5 erfc(x / sqrt 2) = 2^E(x)

E is a degree-6 polynomial: a weighted least-squares fit of log2 Phi(-x) on [0, 6] at 4000 Chebyshev nodes, the residual
weighted by x Phi(-x) + 1e-6 (the GELU error is x q ln 2 times the error of E).  The Gaussian factor of erfc lives in the
polynomial, so the device code needs one transcendental (v_exp_f32) and no reciprocal.

    python tools/fit_gelu.py            # prints the seven coefficients as float32 bit patterns and the emulated max error
"""
import math

import numpy as np

DEGREE = 6
CLAMP = 6.0
NODES = 4000
# the coefficients pasted into csrc/device_utils.h, highest power first (float32 bit patterns)
COMMITTED = (0x3811502c, 0xba4d288b, 0x3c051b28, 0xbd5b0c46, 0xbeeadd98, 0xbf935b1a, 0xbf7fff70)

_erfc = np.frompyfunc(math.erfc, 1, 1)


def phi_neg(x):
    """Phi(-x) = 0.5 erfc(x / sqrt 2) in float64."""
    return 0.5 * _erfc(np.asarray(x, dtype=np.float64) / math.sqrt(2.0)).astype(np.float64)


def fit(degree=DEGREE):
    """-> float32 coefficients of E, highest power first."""
    k = np.arange(NODES)
    t = np.cos(np.pi * (2 * k + 1) / (2 * NODES))          # Chebyshev nodes on [-1, 1]
    x = 0.5 * CLAMP * (t + 1.0)
    q = phi_neg(x)
    c = np.polynomial.chebyshev.chebfit(t, np.log2(q), degree, w=x * q + 1e-6)
    p = np.polynomial.chebyshev.cheb2poly(c)               # power basis in t = x / 3 - 1
    px = np.polynomial.Polynomial(p)(np.polynomial.Polynomial([-1.0, 2.0 / CLAMP]))
    return px.coef[::-1].astype(np.float32)


def bits(coef):
    return tuple(int(b) for b in np.asarray(coef, dtype=np.float32).view(np.uint32))


def from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def gelu_emulated(v, coef):
    """The device arithmetic in float32: one rounding per fma (the double-precision product of two floats is exact)."""
    v = np.asarray(v, dtype=np.float32)
    f64 = np.float64
    x = np.minimum(np.abs(v), np.float32(CLAMP))
    e = np.full_like(x, coef[0])
    for c in coef[1:]:
        e = (e.astype(f64) * x.astype(f64) + f64(c)).astype(np.float32)
    q = np.exp2(e.astype(f64)).astype(np.float32)
    return (-(x.astype(f64)) * q.astype(f64) + np.maximum(v, np.float32(0)).astype(f64)).astype(np.float32)


def gelu_f64(v):
    v = np.asarray(v, dtype=np.float64)
    return v * 0.5 * _erfc(-v / math.sqrt(2.0)).astype(np.float64)


def max_error(coef, lo=-12.0, hi=12.0, n=400001):
    v = np.linspace(lo, hi, n).astype(np.float32)
    edge = np.array([0.0, -0.0, 1e-30, -1e-30, CLAMP, -CLAMP, np.nextafter(np.float32(CLAMP), np.float32(0)), 12.0, -12.0], dtype=np.float32)
    v = np.concatenate([v, edge, -edge])
    return float(np.max(np.abs(gelu_emulated(v, coef).astype(np.float64) - gelu_f64(v.astype(np.float64)))))


def main():
    coef = fit()
    print("degree", DEGREE, "coefficients, highest power first:")
    for c, b in zip(coef, bits(coef)):
        print(f"    0x{b:08x}u   // {float(c):+.9e}")
    print(f"emulated float32 max |error| against float64 GELU on [-12, 12]: {max_error(coef):.3e}")
    if any(COMMITTED):
        print(f"committed coefficients: max |error| {max_error(from_bits(COMMITTED)):.3e}; "
              f"{'same as' if bits(coef) == tuple(COMMITTED) else 'DIFFERENT from'} this fit")


if __name__ == "__main__":
    main()
