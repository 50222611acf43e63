"""float64 numpy restatement of a level-3 convolution chain (csrc/conv_chain.hip): 3 x 1 cross-correlations with zero padding
inside each sample, GroupNorm(1, C) between them (biased variance, eps 1e-5), erf-GELU where a layer asks for it.

    x        (B, HW, C0)            the finished input
    w[i]     (3, C_{i+1}, C_i)      tap t = dh + 1
    gamma[i], beta[i], gelu[i]      the GroupNorm pending on layer i's INPUT, i >= 1 (entry 0 unused)

chain() returns the raw output of every layer, (B, HW, C_{i+1}) each; the last one is what the kernel stores."""
import math

import numpy as np

EPS = 1e-5
_erf = np.vectorize(math.erf, otypes=[np.float64])


def conv3(x, w):
    """out[b, h, n] = sum_t sum_k x[b, h + t - 1, k] w[t, n, k], rows outside [0, HW) read as zero"""
    B, HW, K = x.shape
    xp = np.zeros((B, HW + 2, K))
    xp[:, 1:-1] = x
    out = np.zeros((B, HW, w.shape[1]))
    for t in range(3):
        out += xp[:, t:t + HW] @ w[t].T
    return out


def group_norm(x, gamma, beta):
    mean = x.mean(axis=(1, 2), keepdims=True)
    var = x.var(axis=(1, 2), keepdims=True)
    return (x - mean) / np.sqrt(var + EPS) * gamma + beta


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def chain(x, w, gamma, beta, gelus):
    cur = np.asarray(x, np.float64)
    raw = []
    for i, wi in enumerate(w):
        if i > 0:
            cur = group_norm(cur, np.asarray(gamma[i], np.float64), np.asarray(beta[i], np.float64))
            if gelus[i]:
                cur = gelu(cur)
        cur = conv3(cur, np.asarray(wi, np.float64))
        raw.append(cur)
    return raw


def sums(raw):
    """per sample {sum x, sum x^2} of a raw output: what the statistics slots hold"""
    return np.stack([raw.sum(axis=(1, 2)), (raw * raw).sum(axis=(1, 2))], axis=1)
