"""A numpy restatement of the DPM-Solver++ (2M) sampler (schedulers.DPMSolverMultistepScheduler, csrc/elementwise.hip
solver_step_kernel, the SPDM_DPMPP_2M loop of spdm_sample_run), written from DESIGN.md 8.19 and include/spdm.h alone: the
tables in float64, one update in float32 with every operation rounded on its own, and a float64 loop.  Test support only."""
import numpy as np


def abar(T, beta_start=1e-4, beta_end=0.02):
    return np.cumprod(1.0 - np.linspace(float(beta_start), float(beta_end), T, dtype=np.float64))


def timesteps(T, n):
    ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].astype(np.int64)
    if len(set(ts.tolist())) != n:
        raise ValueError(f"n = {n} repeats a timestep on a grid of {T}")
    return ts


def first_order_rows(n, solver_order=2, lower_order_final=True, euler_at_final=False):
    """flags[i]: loop iteration i is first order by construction."""
    flags = [i == 0 or solver_order == 1 for i in range(n)]
    if euler_at_final or (lower_order_final and n < 15):
        flags[n - 1] = True
    return flags


def table64(T, n, solver_order=2, lower_order_final=True, euler_at_final=False, beta_start=1e-4, beta_end=0.02):
    """(timesteps, (n, 6) float64 rows {sigma_s, alpha_s, k_x, k0f, k0, k1})."""
    a = abar(T, beta_start, beta_end)
    alpha, sigma = np.sqrt(a), np.sqrt(1.0 - a)
    lam = np.log(alpha) - np.log(sigma)
    ts = timesteps(T, n).tolist()
    flags = first_order_rows(n, solver_order, lower_order_final, euler_at_final)
    rows = np.zeros((n, 6), dtype=np.float64)
    for i, s in enumerate(ts):
        t = ts[i + 1] if i + 1 < n else 0
        h = lam[t] - lam[s]
        k0f = -alpha[t] * np.expm1(-h)
        if flags[i]:
            k0, k1 = k0f, 0.0
        else:
            r = (lam[s] - lam[ts[i - 1]]) / h
            k0, k1 = k0f * (1.0 + 1.0 / (2.0 * r)), -k0f / (2.0 * r)
        rows[i] = (sigma[s], alpha[s], sigma[t] / sigma[s], k0f, k0, k1)
    return np.asarray(ts, dtype=np.int64), rows


def table32(*a, **k):
    ts, rows = table64(*a, **k)
    return ts, rows.astype(np.float32)


def step(row, eps, x, x0_prev, first, inpaint=None, dtype=np.float32):
    """One update on (B, H, D) arrays: ``(x', x0)``.  ``first``: run first order whatever the row says.  Each numpy operation
    on arrays of ``dtype`` rounds once, which is the kernel's order: x0; k_x x; + k x0; + k1 x0_prev.  ``inpaint``
    (inp_h, D) or (B, inp_h, D) replaces the first rows of x' (not of x0)."""
    c = np.asarray(row, dtype=dtype)
    eps, x = np.asarray(eps, dtype=dtype), np.asarray(x, dtype=dtype)
    x0 = (x - c[0] * eps) / c[1]
    acc = c[2] * x
    if first or c[5] == 0:
        acc = acc + c[3] * x0
    else:
        acc = acc + c[4] * x0
        acc = acc + c[5] * np.asarray(x0_prev, dtype=dtype)
    if inpaint is not None and inpaint.shape[-2] > 0:
        acc = acc.copy()
        acc[:, :inpaint.shape[-2], :] = inpaint
    return acc.astype(dtype), x0.astype(dtype)


def loop(rows, ts, eps_fn, x, begin=0, end=None, inpaint=None, dtype=np.float64):
    """The sampling loop over iterations [begin, end), first order at ``begin``: the list of iterates after each step.
    ``eps_fn(x, t)`` is the noise predictor."""
    end = len(ts) if end is None else end
    out, x0_prev = [], None
    x = np.asarray(x, dtype=dtype)
    for i in range(begin, end):
        eps = np.asarray(eps_fn(x, int(ts[i])), dtype=dtype)
        x, x0_prev = step(rows[i], eps, x, x0_prev, first=(i == begin), inpaint=inpaint, dtype=dtype)
        out.append(x)
    return out


# the Gaussian toy model: data N(mu, s^2); its exact noise prediction and the exact probability-flow solution
def toy_eps(x, t, a, mu=0.3, s=0.5):
    al, sg = np.sqrt(a[t]), np.sqrt(1.0 - a[t])
    return sg * (x - al * mu) / (al * al * s * s + sg * sg)


def toy_exact(x_T, t, T_start, a, mu=0.3, s=0.5):
    al, sg = np.sqrt(a[t]), np.sqrt(1.0 - a[t])
    aT, sT = np.sqrt(a[T_start]), np.sqrt(1.0 - a[T_start])
    return al * mu + np.sqrt(al * al * s * s + sg * sg) / np.sqrt(aT * aT * s * s + sT * sT) * (x_T - aT * mu)
