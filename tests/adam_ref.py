"""Float64 statement of one optimiser step as ``spdm_adam_step`` specifies it (include/spdm.h): global-norm
gradient clipping with ``clip_grad_norm_``'s semantics, then torch's Adam with ``amsgrad=False``, ``weight_decay=0``.  Plain
numpy; tests/test_adam_reference.py pins it to ``torch.optim.Adam`` + ``clip_grad_norm_`` run in float64, and the GPU tests
measure both the HIP step and torch's fp32 step against it."""
import numpy as np


def grad_norm(grads):
    """sqrt of the sum of squares over ALL segments, in float64."""
    return float(np.sqrt(sum(float(np.sum(np.square(np.asarray(g, np.float64)))) for g in grads)))


def clip_coef(norm, max_norm):
    """``clip_grad_norm_``: clamp(max_norm / (norm + 1e-6), max=1); None / <= 0: no clipping."""
    if not max_norm or max_norm <= 0:
        return 1.0
    c = float(max_norm) / (norm + 1e-6)
    return 1.0 if c > 1.0 else c           # (a NaN stays a NaN)


def adam_step(params, grads, exp_avgs, exp_avg_sqs, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=None):
    """One step over the segments (lists of float64 arrays, updated in place).  ``step`` >= 1 counts this step.  The
    gradients are only read.  Returns the gradient norm (before clipping)."""
    beta1, beta2 = betas
    norm = grad_norm(grads)
    coef = clip_coef(norm, max_norm)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        gc = np.asarray(g, np.float64) * coef
        m *= beta1
        m += (1.0 - beta1) * gc
        v *= beta2
        v += (1.0 - beta2) * gc * gc
        p -= (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return norm


class RefAdam:
    """The reference as an optimiser over float64 copies of the segments' initial values."""

    def __init__(self, params, betas=(0.9, 0.999), eps=1e-8):
        self.p = [np.array(p, np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.betas, self.eps, self.t = betas, eps, 0
        self.norm = None

    def step(self, grads, lr, max_norm=None):
        self.t += 1
        self.norm = adam_step(self.p, grads, self.m, self.v, self.t, lr=lr, betas=self.betas, eps=self.eps, max_norm=max_norm)
        return self.norm


# ---- the inputs and the tolerance rule the GPU tests share -----------------------------------------------------------------
def zero_block(n):
    """The block of a gradient that is exactly zero in every step: [n / 4, n / 2) (empty for n = 1)."""
    return slice(n // 4, n // 2)


def make_inputs(sizes, steps=5, seed=0):
    """p ~ 0.05 N(0,1); per step g ~ N(0,1) 10^U(-6,0) elementwise with ``zero_block`` exactly zero.  float32 arrays."""
    rng = np.random.default_rng(seed + 1000 * len(sizes) + sum(sizes))
    params = [(0.05 * rng.standard_normal(n)).astype(np.float32) for n in sizes]
    grads = []
    for _ in range(steps):
        gs = []
        for n in sizes:
            g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6.0, 0.0, n)).astype(np.float32)
            g[zero_block(n)] = 0.0
            gs.append(g)
        grads.append(gs)
    return params, grads


def within_rule(x_dev, x_torch, x64):
    """The accuracy rule: max|dev - x64| <= 2 max|torch32 - x64| + 2^-24 max|x64|.  Returns (ok, err_dev, err_torch, bound):
    the factor 2 is the margin for two correct fp32 evaluations of one formula in different operation orders, the last term
    one fp32 rounding of the largest value."""
    x64 = np.asarray(x64, np.float64)
    e_dev = float(np.max(np.abs(np.asarray(x_dev, np.float64) - x64)))
    e_torch = float(np.max(np.abs(np.asarray(x_torch, np.float64) - x64)))
    bound = 2.0 * e_torch + 2.0 ** -24 * float(np.max(np.abs(x64)))
    return bool(np.isfinite(e_dev) and e_dev <= bound), e_dev, e_torch, bound
