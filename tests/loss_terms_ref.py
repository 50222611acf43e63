"""numpy restatement of csrc/train_metrics.hip (spdm_loss_terms) in the kernel's exact summation order, so that the kernel's
terms can be compared bit for bit: numpy's float64 scalar arithmetic rounds every operation on its own, as the kernel does.

Per sample of n = H x D elements (row-major): element e belongs to partial e mod 64; a partial starts at 0.0 and adds
((double)noise[e] - (double)eps[e])^2 for its elements in ascending e; the 64 partials are combined by the tree
``for off in 32, 16, 8, 4, 2, 1: p[i] = p[i] + p[i + off] (i < off)``; the term is p[0] / (double)n."""
import numpy as np

LANES = 64


def loss_terms(eps: np.ndarray, noise: np.ndarray) -> np.ndarray:
    """(B,) float64 terms of fp32 ``eps`` / ``noise`` of shape (B, ...)."""
    assert eps.dtype == np.float32 and noise.dtype == np.float32 and eps.shape == noise.shape
    B = eps.shape[0]
    e64 = eps.reshape(B, -1).astype(np.float64)
    n64 = noise.reshape(B, -1).astype(np.float64)
    n = e64.shape[1]
    d = n64 - e64
    sq = d * d                                        # one rounding each, as the kernel's d * d
    rows = -(-n // LANES)
    padded = np.zeros((B, rows * LANES), dtype=np.float64)
    padded[:, :n] = sq
    p = np.zeros((B, LANES), dtype=np.float64)
    for r in range(rows):                             # lane l adds elements l, l + 64, ... in ascending order; a missing
        p = p + padded[:, r * LANES:(r + 1) * LANES]  # element adds +0.0, which changes no bit of a non-negative partial
    off = LANES // 2
    while off >= 1:
        p = p[:, :off] + p[:, off:2 * off]
        off //= 2
    return p[:, 0] / np.float64(n)


def pass_mean(terms: np.ndarray) -> np.float64:
    """spdm_eval_reduce's d_mean over (N, 1) terms with runs = 1, in its order (csrc/evaluation.hip): blocks of 1024 rows; in a
    block thread t adds rows t, t + 256, ... (four at most), each wave of 64 threads is combined by the same shuffle tree, the
    four waves are added in wave order, the blocks in block order; the total is divided by N."""
    terms = np.asarray(terms, dtype=np.float64).reshape(-1)
    N = terms.size
    total = None
    for b0 in range(0, N, 1024):
        blk = np.zeros(1024, dtype=np.float64)
        chunk = terms[b0:b0 + 1024]
        blk[:chunk.size] = chunk
        acc = np.zeros(256, dtype=np.float64)
        for i in range(4):
            acc = acc + blk[i * 256:(i + 1) * 256]
        w = acc.reshape(4, 64)
        off = 32
        while off >= 1:
            w = w[:, :off] + w[:, off:2 * off]
            off //= 2
        tot = w[0, 0]
        for k in range(1, 4):
            tot = tot + w[k, 0]
        total = tot if total is None else total + tot
    return total / np.float64(N)
