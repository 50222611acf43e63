"""Plain CPU references of ONE training launch (spdm_op_train, include/spdm.h), for tests only: numpy (torch for erf), nothing
from the project.

For every op:
  ref64(op, inp)      the operation in float64, written from its definition, on the float32 values the kernel is given
                      (every comparison -- the pooling argmax -- is then exact and the kernel's own);
  scale64(op, inp)    the same expression with every term in absolute value: the S of the tolerance;
  ref32(op, inp)      the same formulas in float32 with every sum taken SEQUENTIALLY in float32 (np.add.accumulate or an explicit
                      loop): the worst fixed order a kernel could have chosen;
  MUTANTS[op]         float64 models of the mistakes the kernel could make (ref64(op, inp, mutant=name)).
All four return a dict of named outputs; every element of every output is compared.

Tolerance, per element: |got - ref64| <= TAU * S with TAU = 4 * max over elements of |ref32 - ref64| / S, from the references
alone (tau()); the factor 4 covers the device's own fixed summation order and math library.  Ops with a math-library call have
a floor TAU >= FLOOR_U[op] * u, u = 2^-24 (the count is written beside FLOOR_U).  Where S is zero the element must be equal
(exact zeros of padded lanes, side columns, zero gradients; copies).

cases(op) is the case table (shapes and data flavours) the CPU and GPU tests share; make_inputs(op, case) the data.
"""
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
WGRAD_BUDGET = 16 << 20            # floats of weight-gradient partial slabs (the training pass's budget)
LN_BWD_ROWS = 64
EPS = 1e-5
# S of a leaf that comes out of exp, tanh or a reciprocal of them counts |leaf| + TINY: below the normal range (2^-126) a
# float32 value has no relative precision, with or without flush to zero, and may be lost entirely; in units of u that is 2^-102
TINY = 2.0 ** -102

OPS = ("wgrad", "wgrad_mapped", "colsum", "gn_stats", "gn_bwd", "film_bwd", "mse", "pool_bwd", "up_bwd", "mish_bwd",
       "ln_fwd", "ln_bwd", "gelu_bwd", "attn_fwd_lse", "attn_bwd", "gn_bwd_mapped", "simple_tail_bwd", "silu_bwd")

# Floors of TAU in units of u for the ops with math-library calls: roundings on the longest dependency chain of one element
# (1 u each) plus the documented bounds of the device functions on it (HIP math API: erff 2 ulp, expf 1, tanhf 2, log1pf 1,
# logf 1, sqrtf / division correctly rounded; k ulp = 2 k u).
FLOOR_U = {
    # v / sqrt2 (1), erff (4), 1 + (1), v v (1), expf (2), c * (1), v * pdf (1), cdf + (1), dh * (1)
    "gelu_bwd": 13,
    # the sum (1 per add is in ref32); expf (2), log1pf (2), tanhf (4), expf (2), 1 + (1), 1 / (1), th th (1), 1 - (1),
    # x * (1), * sg (1), th + (1), s * (1)
    "mish_bwd": 18,
    # expf (2), 1 + (1), 1 / (1), 1 - sg (1), x * (1), 1 + (1), sg * (1), ds * (1)
    "silu_bwd": 9,
    # gn_bwd with GELU': xh (2), gamma xh + beta (2), gelu' as gelu_bwd (11), g * (1), * gamma (1), - m1 (1), xh m2 (1), - (1), rs * (1)
    "gn_bwd": 21, "gn_bwd_mapped": 21,
    # q scale (1), dot (in ref32), - m (1), expf (2) amplified by the argument (in ref32), p v (1), 1 / l (1), * inv (1), logf (2), m + (1)
    "attn_fwd_lse": 10,
    # q scale (1), - lse (1), expf (2), dO.V - D (1), p * (1), ds k (1), * scale (1)
    "attn_bwd": 8,
    # mean: / C (1); d = v - mu (1), d d (1), / C (1), + eps (1), sqrtf (1), 1 / (1), * rs (1), * g (1), + b (1)
    "ln_fwd": 10,
    "gn_stats": 4,                 # fp64 sums; / cnt, sqrt, 1 /, the float32 store (1 each)
}


# ---- helpers -------------------------------------------------------------------------------------------------------------
def ssum(a, axis, seq):
    """Sum over `axis` (int or tuple, in C order); seq: sequentially in a's own precision."""
    axis = (axis,) if isinstance(axis, int) else tuple(axis)
    if not seq:
        return a.sum(axis=axis)
    axis = tuple(ax % a.ndim for ax in axis)
    a = np.moveaxis(a, axis, tuple(range(a.ndim - len(axis), a.ndim)))
    a = a.reshape(a.shape[:a.ndim - len(axis)] + (-1,))
    return np.add.accumulate(a, axis=-1)[..., -1]


def mm_t(a, b, seq):
    """sum_m a[m, i] b[m, j] -> [i, j]; seq: one product and one add per row, in order, in the arrays' precision."""
    if not seq:
        return a.T @ b
    acc = np.zeros((a.shape[1], b.shape[1]), a.dtype)
    for m in range(a.shape[0]):
        acc += a[m][:, None] * b[m][None, :]
    return acc


def _erf(x):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return (1 / (1 + np.exp(-x))).astype(x.dtype)


def _pdf(v):
    return (np.exp(-0.5 * v * v) * v.dtype.type(1 / math.sqrt(2 * math.pi))).astype(v.dtype)


def _gelu_grad(v, ab=False, mutant=None):
    e = _erf(v * v.dtype.type(math.sqrt(0.5)))
    if ab:
        return 0.5 + 0.5 * np.abs(e) + np.abs(v) * (_pdf(v) + TINY)
    cdf = 0.5 * (1 + e)
    if mutant == "saturate_early":
        cdf = np.where(v > 2, 1.0, cdf).astype(v.dtype)
    return cdf if mutant == "drop_xpdf" else cdf + v * _pdf(v)


def wgrad_geometry(M, taps, Co, Ci):
    """(chunks, rows per chunk) of the weight gradient's row split: min(2048 / tiles, M / 64, budget), rows rounded up to 4."""
    tiles = ((Co + 63) // 64) * ((Ci + 63) // 64) * taps
    n = max(1, 2048 // tiles)
    n = min(n, max(1, M // 64))
    n = min(n, max(1, WGRAD_BUDGET // (taps * Co * Ci)))
    rows = (M + n - 1) // n
    return n, (rows + 3) // 4 * 4


def ln_bwd_blocks(rows):
    return (rows + LN_BWD_ROWS - 1) // LN_BWD_ROWS


# ---- the ops: f(inp, dt, ab, seq, mutant) -> {name: array} ------------------------------------------------------------------
def _A(inp, dt, ab, *names):
    out = []
    for n in names:
        v = np.asarray(inp[n]).astype(dt)
        out.append(np.abs(v) if ab else v)
    return out


def _wgrad_core(dy, x, B, H, W, taps, conv9, dt, seq, mutant, chunks):
    """dW[co, ci, ky, kx] = sum_{b, y, x} dy[b, y, x, co] xpad[b, y + ky - 1, x + kx - 1, ci] (zero padding)."""
    M, Co, Ci = B * H * W, dy.shape[1], x.shape[1]
    dy = dy.copy()
    nch, rows = chunks
    if mutant == "drop_chunk_last_row":
        for c in range(nch):
            m1 = min(M, (c + 1) * rows)
            if m1 > c * rows:
                dy[m1 - 1] = 0
    elif mutant == "drop_partial_kstep":
        for c in range(nch):
            m0, m1 = c * rows, min(M, (c + 1) * rows)
            if m1 > m0:
                dy[m1 - (m1 - m0) % 4:m1] = 0
    elif mutant == "drop_chunk":
        c = 1 if nch > 1 else 0
        dy[c * rows:min(M, (c + 1) * rows)] = 0
    if taps == 1:
        return mm_t(dy, x, seq)
    out = np.zeros((Co, Ci, 3, 3), dt)
    m = np.arange(M)
    b, p = m // (H * W), m % (H * W)
    yy, xx = p // W, p % W
    for ky in range(3):
        for kx in range(3):
            if taps == 3 and kx != 1 and mutant != "no_xbound":
                continue                   # W == 1: the side taps read padding only
            ys, xs = yy + ky - 1, xx + kx - 1
            ok = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
            src = b * H * W + ys * W + xs
            if mutant == "no_xbound":      # the tap wraps into the neighbouring map row (of the same sample)
                flat = ys * W + xs
                ok = (ys >= 0) & (ys < H) & (flat >= 0) & (flat < H * W)
            elif mutant == "cross_sample":  # no y bound: the tap reads the neighbouring sample
                ok = (xs >= 0) & (xs < W) & (src >= 0) & (src < M)
            xs_rows = np.where(ok[:, None], x[np.clip(src, 0, M - 1)], 0).astype(dt)
            out[:, :, ky, kx] = mm_t(dy, xs_rows, seq)
    if mutant == "side_column":
        out[:, :, :, 0] = out[:, :, :, 1]
    return out if conv9 else out[:, :, 1, 1]


def _wgrad(inp, dt, ab, seq, mutant):
    B, H, W, taps, Co, Ci, conv9, ldy, ldx = (inp[k] for k in ("B", "H", "W", "taps", "Co", "Ci", "conv9", "ldy", "ldx"))
    M = B * H * W
    dyb, xb = _A(inp, dt, ab, "dy", "x")
    dy, x = dyb[:, :Co], xb[:, :Ci]
    if mutant == "ldx_as_width":
        x = xb.ravel()[:M * Ci].reshape(M, Ci)
    if mutant == "ldy_as_width":
        dy = dyb.ravel()[:M * Co].reshape(M, Co)
    return {"dst": _wgrad_core(dy, x, B, H, W, taps, conv9, dt, seq, mutant, wgrad_geometry(M, taps, Co, Ci))}


def _wgrad_mapped(inp, dt, ab, seq, mutant):
    B, H, W, taps, Co, Ci = (inp[k] for k in ("B", "H", "W", "taps", "Co", "Ci"))
    dy, x = _A(inp, dt, ab, "dy", "x")
    po, pi = np.asarray(inp["pos_o"]), np.asarray(inp["pos_i"])
    if mutant == "map_ignored":
        po, pi = np.arange(len(po)), np.arange(len(pi))
    return {"dst": _wgrad_core(dy[:, po], x[:, pi], B, H, W, taps, 1, dt, seq, mutant, wgrad_geometry(B * H * W, taps, Co, Ci))}


def _colsum(inp, dt, ab, seq, mutant):
    """dst[c] = sum_m src[m, c]: columns [off, off + C) of a buffer whose rows are ld floats."""
    (buf,) = _A(inp, dt, ab, "buf")
    M, C, off = inp["M"], inp["C"], inp["off"]
    s = buf[:, off:off + C]
    if mutant == "ld_as_width":
        s = buf.ravel()[off:off + M * C].reshape(M, C)
    if mutant == "drop_last_row":
        s = s[:-1] if M > 1 else s * 0
    return {"dst": ssum(s, 0, seq)}


def _gn_stats(inp, dt, ab, seq, mutant):
    """GroupNorm(1, C) statistics of the REAL channels of each sample: mean, 1 / sqrt(var + eps)."""
    y = np.asarray(inp["y"]).astype(dt)                   # [B, HW, C]
    pos = np.asarray(inp["pos"])
    B = y.shape[0]
    real = y[:, :, pos].reshape(B, -1)
    cnt = real.shape[1]
    if mutant == "divisor_n":
        cnt = y.shape[1] * y.shape[2]
    mean = ssum(real, 1, seq) / dt(cnt)
    dev = real - mean[:, None]
    var = ssum(dev * dev, 1, seq) / dt(cnt)
    if mutant == "divisor_n":
        var = ssum(real * real, 1, seq) / dt(cnt) - mean * mean
    rstd = 1 / np.sqrt(var + dt(EPS))
    if not ab:
        return {"mean": mean, "rstd": rstd.astype(dt)}
    s_mean = np.abs(real).sum(1) / cnt
    s_var = ((np.abs(real) + np.abs(mean)[:, None]) ** 2).sum(1) / cnt
    return {"mean": s_mean, "rstd": rstd + 0.5 * rstd ** 3 * s_var}


def _gn_bwd_any(inp, dt, ab, seq, mutant, pos):
    """out = [GELU](gamma xh + beta), xh = (y - mean) rstd over the real lanes of a sample:
    dy = rstd (gg - mean(gg) - xh mean(gg xh)), gg = g [GELU'(gamma xh + beta)] gamma; dgb = {sum_p g' xh, sum_p g'}."""
    y, g, gamma, beta, mean, rstd = (np.asarray(inp[k]).astype(dt) for k in ("y", "g", "gamma", "beta", "mean", "rstd"))
    B, HW, C = y.shape
    real = np.zeros(C, bool)
    real[pos] = True
    xh = (y - mean[:, None, None]) * rstd[:, None, None]
    gp = np.abs(g) if ab else g
    if inp["gelu"]:
        arg = xh if mutant == "gelu_at_xh" else gamma * xh + beta
        gp = (gp * _gelu_grad(arg.astype(dt), ab)).astype(dt)
    ga = np.abs(gamma) if ab else gamma
    xa = np.abs(xh) if ab else xh
    gg = gp * ga
    cnt = HW * (C if mutant == "padded_lane" else int(real.sum()))
    lanes = np.ones(C, bool) if mutant == "padded_lane" else real
    m1 = ssum(gg[:, :, lanes], (1, 2), seq) / dt(cnt)
    m2 = ssum((gg * xa)[:, :, lanes], (1, 2), seq) / dt(cnt)
    if mutant == "drop_xh_term":
        m2 = m2 * 0
    t1, t2 = m1[:, None, None], xa * m2[:, None, None]
    dy = rstd[:, None, None] * ((gg + t1 + t2) if ab else (gg - t1 - t2))
    dgb = np.stack([ssum(gp * xa, 1, seq), ssum(gp, 1, seq)], axis=-1)       # [B, C, 2]
    dy[:, :, ~real] = 0
    dgb[:, ~real] = 0
    return {"dy": dy.astype(dt), "dgb": dgb.astype(dt)}


def _gn_bwd(inp, dt, ab, seq, mutant):
    return _gn_bwd_any(inp, dt, ab, seq, mutant, np.arange(inp["y"].shape[2]))


def _gn_bwd_mapped(inp, dt, ab, seq, mutant):
    return _gn_bwd_any(inp, dt, ab, seq, mutant, np.asarray(inp["pos"]))


def _film_bwd(inp, dt, ab, seq, mutant):
    """out = s (z + e) + f (film None: out = z + e), e = temb[t_b]: dz = s dout, de = s sum_p dout, ds = sum_p dout (z + e),
    df = sum_p dout; dfilm = [ds | df]."""
    z, temb, dout = _A(inp, dt, ab, "z", "temb", "dout")
    B, HW, C = z.shape
    t = np.asarray(inp["t"])
    e = temb[t if len(t) == B else np.repeat(t, B)]                           # [B, C]
    film = inp.get("film")
    sc = np.ones((B, C), dt) if film is None else _A(inp, dt, ab, "film")[0][:, :C]
    sd = ssum(dout, 1, seq)
    out = {"dz": sc[:, None, :] * dout, "de": sd if mutant == "de_no_scale" else sc * sd}
    if film is not None:
        ze = z if mutant == "ds_without_e" else z + e[:, None, :]
        out["dfilm"] = np.concatenate([ssum(dout * ze, 1, seq), sd], axis=1)
    return out


def _mse(inp, dt, ab, seq, mutant):
    """loss = mean over the unpadded lanes of (eps - noise)^2; deps_pad = d loss / d eps on the padded map; eps_out = eps
    (an optional output: absent where the case says eps_out = 0)."""
    out = _mse_all(inp, dt, ab, seq, mutant)
    if not inp.get("eps_out", 1):
        del out["eps_out"]
    return out


def _mse_all(inp, dt, ab, seq, mutant):
    B, H0, D, Hp, Wp, lh, lw = (inp[k] for k in ("B", "H0", "D", "Hp", "Wp", "lh", "lw"))
    eps_pad, noise = (np.asarray(inp[k]).astype(dt) for k in ("eps_pad", "noise"))
    eps = eps_pad[:, lh:lh + H0, lw:lw + D]
    n = B * Hp * Wp if mutant == "padded_n" else B * H0 * D
    if ab:
        diff = np.abs(eps) + np.abs(noise)
        deps = np.zeros_like(eps_pad)
        deps[:, lh:lh + H0, lw:lw + D] = dt(2) / dt(n) * diff
        return {"loss": (diff * diff).sum().reshape(1) / n, "deps_pad": deps, "eps_out": np.zeros_like(eps)}
    diff = eps - noise
    full = eps_pad.copy()
    full[:, lh:lh + H0, lw:lw + D] = diff
    deps = np.zeros_like(eps_pad)
    deps[:, lh:lh + H0, lw:lw + D] = dt(2) / dt(n) * diff
    sq = diff * diff
    if mutant == "padded_lane":
        deps, sq = dt(2) / dt(n) * full, full * full
    return {"loss": (ssum(sq.reshape(-1), 0, seq) / dt(n)).reshape(1), "deps_pad": deps, "eps_out": eps.copy()}


def _pool_bwd(inp, dt, ab, seq, mutant):
    """Backward of MaxPool2d(2): the window's gradient goes to its FIRST maximum in scan order, added to din.  One correctly
    rounded add per element: the float32 rounding of the exact sum is every IEEE implementation's answer, so that is returned."""
    x = np.asarray(inp["in"])                                                  # comparisons on the float32 values
    B, H, W, C = x.shape
    dout, din = _A(inp, F64, ab, "dout", "din")
    win = x.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)
    if mutant == "last_max":
        best = 3 - np.argmax(win[:, :, :, ::-1], axis=3)
    else:
        best = np.argmax(win, axis=3)                                          # the first occurrence; +0.0 == -0.0
    hit = (np.arange(4)[None, None, None, :, None] == best[:, :, :, None, :])
    scat = (hit * dout[:, :, :, None, :]).reshape(B, H // 2, W // 2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if ab:
        return {"din": np.zeros_like(scat)}                                    # TAU = 0: equality
    if mutant == "assign":
        hit_full = hit.reshape(B, H // 2, W // 2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
        return {"din": np.where(hit_full, scat, din).astype(F32).astype(F64)}
    return {"din": (din + scat).astype(F32).astype(F64)}


def _up_matrix(n, dt):
    """[2n, n] weights of a bilinear x2, align_corners=True resampling."""
    m = np.zeros((2 * n, n), dt)
    scale = dt(n - 1) / dt(2 * n - 1) if n > 1 else dt(0)
    for o in range(2 * n):
        src = scale * dt(o)
        i0 = int(src)
        i1 = min(i0 + 1, n - 1)
        l1 = src - dt(i0)
        m[o, i0] += dt(1) - l1
        m[o, i1] += l1
    return m


def _up_bwd(inp, dt, ab, seq, mutant):
    """dx[b, iy, ix, c] += sum_{oy, ox} wy[oy, iy] wx[ox, ix] dcat[b, oy, ox, c] (channels [0, C) of rows of ld)."""
    B, h, w, C = (inp[k] for k in ("B", "h", "w", "C"))
    dcat, dx = _A(inp, dt, ab, "dcat", "dx")
    d = dcat.reshape(B, 2 * h, 2 * w, -1)[..., :C]
    wy, wx = _up_matrix(h, dt), _up_matrix(w, dt)

    def shorten(m, lo):
        m = m.copy()
        for i in range(m.shape[1]):
            nz = np.nonzero(m[:, i])[0]
            m[nz[0] if lo else nz[-1], i] = 0
        return m
    if mutant == "window_short_lo":
        wy, wx = shorten(wy, True), shorten(wx, True)
    if mutant == "window_short_hi":
        wy, wx = shorten(wy, False), shorten(wx, False)
    if mutant == "nin1_one_output":
        if h == 1:
            wy[1] = 0
        if w == 1:
            wx[1] = 0
    # r[b, oy, ix, c] = sum_ox wx d, then s = sum_oy wy r: the terms in output order
    r = ssum(d[:, :, :, None, :] * wx[None, None, :, :, None], 2, seq)
    s = ssum(r[:, :, None, :, :] * wy[None, :, :, None, None], 1, seq)
    return {"dx": s if mutant == "assign" else dx + s}


def _mish_bwd(inp, dt, ab, seq, mutant):
    """grad = Mish'(x) sum_k dm[k], Mish'(x) = tanh(sp) + x (1 - tanh(sp)^2) sigmoid(x), sp = log(1 + e^x)."""
    dm, = _A(inp, dt, ab, "dm")
    x = np.asarray(inp["cond"]).astype(dt)
    s = ssum(dm[:, :, :x.shape[1]], 0, seq)
    sp = np.logaddexp(dt(0), x).astype(dt)
    if mutant == "saturate_early":
        sp = np.where(x > 0.2, x, sp).astype(dt)
    th, sg = np.tanh(sp), _sigmoid(x)
    if ab:
        return {"grad_cond": s * (np.abs(th) + TINY + np.abs(x) * (1 + th * th) * (sg + TINY))}
    return {"grad_cond": s * th if mutant == "drop_xpdf" else s * (th + x * (1 - th * th) * sg)}


def _silu_bwd(inp, dt, ab, seq, mutant):
    """grad = ds SiLU'(x), SiLU'(x) = sg (1 + x (1 - sg))."""
    ds, = _A(inp, dt, ab, "ds")
    x = np.asarray(inp["cond"]).astype(dt)
    ds = ds[:, :x.shape[1]]
    sg = _sigmoid(x)
    if mutant == "saturate_early":
        sg = np.where(x > 2, 1.0, sg).astype(dt)
    if ab:
        return {"grad_cond": ds * ((sg + TINY) * (1 + np.abs(x) * (1 + sg)))}
    return {"grad_cond": ds * sg if mutant == "drop_xpdf" else ds * (sg * (1 + x * (1 - sg)))}


def _gelu_bwd(inp, dt, ab, seq, mutant):
    """du = dh (Phi(u) + u phi(u))."""
    dh, = _A(inp, dt, ab, "dh")
    u = np.asarray(inp["u"]).astype(dt)
    return {"du": dh * _gelu_grad(u, ab, mutant)}


def _ln_fwd(inp, dt, ab, seq, mutant):
    x, g, b = (np.asarray(inp[k]).astype(dt) for k in ("x", "g", "b"))
    C = x.shape[1]
    mean = ssum(x, 1, seq) / dt(C)
    dev = x - mean[:, None]
    var = ssum(dev * dev, 1, seq) / dt(C)
    if mutant == "no_eps":
        rstd = 1 / np.sqrt(var + dt(1e-30))
    else:
        rstd = 1 / np.sqrt(var + dt(EPS))
    rstd = rstd.astype(dt)
    if mutant == "drop_last_lane":
        mean = ssum(x[:, :-1], 1, seq) / dt(C)
    if not ab:
        return {"y": (x - mean[:, None]) * rstd[:, None] * g + b, "mean": mean, "rstd": rstd}
    s_mean = np.abs(x).sum(1) / C
    s_var = ((np.abs(x) + s_mean[:, None]) ** 2).sum(1) / C
    s_rstd = rstd + 0.5 * rstd ** 3 * s_var
    s_y = ((np.abs(x) + s_mean[:, None]) * rstd[:, None] + np.abs(dev) * (s_rstd - rstd)[:, None]) * np.abs(g) + np.abs(b)
    return {"y": s_y, "mean": s_mean, "rstd": s_rstd}


def _ln_bwd(inp, dt, ab, seq, mutant):
    """dx = rstd (gg - mean(gg) - xh mean(gg xh)) (+ add), gg = gy gamma; part[block] = [sum gy xh | sum gy] over 64-row blocks."""
    x, mean, rstd, gamma, gy = (np.asarray(inp[k]).astype(dt) for k in ("x", "mean", "rstd", "gamma", "gy"))
    rows, C = x.shape
    xh = (x - mean[:, None]) * rstd[:, None]
    if ab:
        xh, gamma, gy = np.abs(xh), np.abs(gamma), np.abs(gy)
    gg = gy * gamma
    s1 = ssum(gg, 1, seq) / dt(C)
    s2 = ssum(gg * xh, 1, seq) / dt(C)
    if mutant == "drop_xh_term":
        s2 = s2 * 0
    dx = rstd[:, None] * ((gg + s1[:, None] + xh * s2[:, None]) if ab else (gg - s1[:, None] - xh * s2[:, None]))
    if inp.get("add") is not None and mutant != "drop_add":
        dx = dx + _A(inp, dt, ab, "add")[0]
    nb = ln_bwd_blocks(rows)
    part = np.zeros((nb, 2 * C), dt)
    for k in range(nb):
        r0, r1 = k * LN_BWD_ROWS, min(rows, (k + 1) * LN_BWD_ROWS)
        if mutant == "ragged_block_missing" and r1 - r0 < LN_BWD_ROWS:
            continue
        part[k, :C] = ssum((gy * xh)[r0:r1], 0, seq)
        part[k, C:] = ssum(gy[r0:r1], 0, seq)
    return {"dx": dx, "part": part}


def _heads(qkv, B, L, C, heads):
    d = C // heads
    t = qkv.reshape(B, L, 3, heads, d).transpose(2, 0, 3, 1, 4)               # [3, B, heads, L, d]
    return t[0], t[1], t[2]


def _dot_last(a, b, seq):
    """sum_k a[..., i, k] b[..., j, k] -> [..., i, j]"""
    if not seq:
        return a @ np.swapaxes(b, -1, -2)
    acc = np.zeros(a.shape[:-1] + (b.shape[-2],), a.dtype)
    for k in range(a.shape[-1]):
        acc += a[..., :, None, k] * b[..., None, :, k]
    return acc


def _wsum(p, v, seq):
    """sum_j p[..., i, j] v[..., j, k] -> [..., i, k], j in order"""
    if not seq:
        return p @ v
    acc = np.zeros(p.shape[:-1] + (v.shape[-1],), p.dtype)
    for j in range(p.shape[-1]):
        acc += p[..., :, j, None] * v[..., None, j, :]
    return acc


def _attn_fwd_lse(inp, dt, ab, seq, mutant):
    """out = softmax(q k^T / sqrt(d)) v per (sample, head); lse = log sum_j exp(score)."""
    B, L, C, heads = (inp[k] for k in ("B", "L", "C", "heads"))
    q, k, v = _heads(np.asarray(inp["qkv"]).astype(dt), B, L, C, heads)
    if mutant == "heads_swapped":
        k = k[:, ::-1]
    d = C // heads
    scale = dt(1) / np.sqrt(dt(d))
    s = _dot_last((q * scale).astype(dt), k, seq)
    if mutant == "first256":
        s, v = s[..., :256], v[..., :256, :]
    with np.errstate(over="ignore", invalid="ignore"):
        m = np.zeros_like(s.max(-1)) if mutant == "lse_no_max" else s.max(-1)
        p = np.exp(s - m[..., None]).astype(dt)
        l = ssum(p, -1, seq)
        if ab:
            sa = _dot_last(np.abs(q * scale), np.abs(k), False).max(-1)
            out, lse = _wsum(p + TINY, np.abs(v), False) / l[..., None], sa + np.abs(np.log(l))
        else:
            out, lse = _wsum(p, v, seq) * (dt(1) / l)[..., None], m + np.log(l)
    return {"out": out.transpose(0, 2, 1, 3).reshape(B, L, C).astype(dt), "lse": lse.astype(dt)}


def _attn_bwd(inp, dt, ab, seq, mutant):
    """P = exp(score - lse); dS = P o (dO V^T - rowsum(dO o O)); dQ = dS K / sqrt(d), dK = dS^T Q / sqrt(d), dV = P^T dO."""
    B, L, C, heads = (inp[k] for k in ("B", "L", "C", "heads"))
    d = C // heads
    q, k, v = _heads(np.asarray(inp["qkv"]).astype(dt), B, L, C, heads)
    hd = lambda t: np.asarray(t).astype(dt).reshape(B, L, heads, d).transpose(0, 2, 1, 3)
    o, do = hd(inp["out"]), hd(inp["dout"])
    lse = np.asarray(inp["lse"]).astype(dt)
    if mutant == "heads_swapped":
        k = k[:, ::-1]
    scale = dt(1) / np.sqrt(dt(d))
    qs = (q * scale).astype(dt)
    p = np.exp(_dot_last(qs, k, seq) - lse[..., None]).astype(dt)
    if ab:
        p, do, o, v, k, qs = p + TINY, np.abs(do), np.abs(o), np.abs(v), np.abs(k), np.abs(qs)
    di = ssum(do * o, -1, seq)
    if mutant == "drop_rowsum":
        di = di * 0
    dov = _dot_last(do, v, seq)
    ds = p * ((dov + di[..., None]) if ab else (dov - di[..., None]))
    pq, dsq = p, ds
    if mutant == "first256":
        ds = ds.copy(); ds[..., 256:] = 0
        pq, dsq = p.copy(), ds.copy()
        pq[..., 256:, :] = 0; dsq[..., 256:, :] = 0
    dq = _wsum(ds, k, seq) * (dt(1) if mutant == "no_scale_dq" else scale)
    dk = _wsum(np.swapaxes(dsq, -1, -2), qs, seq)
    dv = _wsum(np.swapaxes(pq, -1, -2), do, seq)
    out = np.stack([dq, dk, dv], 0).transpose(1, 3, 0, 2, 4).reshape(B, L, 3 * C)
    return {"dqkv": out.astype(dt)}


def _simple_tail_bwd(inp, dt, ab, seq, mutant):
    """dz = dout[:, :, :Cr] then zeros up to Cz; dtemb = sum_p dout[:, :, :Cr]; dcemb = sum_p dout[:, :, Cr:Cr + 32]."""
    dout, = _A(inp, dt, ab, "dout")
    Cr, Cz = inp["Cr"], inp["Cz"]
    dz = dout[:, :, :Cz].copy()
    if mutant != "dz_pad_kept":
        dz[:, :, Cr:] = 0
    src = dout[:, :-1] if mutant == "drop_last_row" else dout
    s = ssum(src, 1, seq) if src.shape[1] else dout[:, 0] * 0
    if ab:
        dz = dz * 0                                                            # a copy: equality
    return {"dz": dz, "dtemb": s[:, :Cr], "dcemb": s[:, Cr:Cr + 32]}


_IMPL = {"wgrad": _wgrad, "wgrad_mapped": _wgrad_mapped, "colsum": _colsum, "gn_stats": _gn_stats, "gn_bwd": _gn_bwd,
         "film_bwd": _film_bwd, "mse": _mse, "pool_bwd": _pool_bwd, "up_bwd": _up_bwd, "mish_bwd": _mish_bwd, "ln_fwd": _ln_fwd,
         "ln_bwd": _ln_bwd, "gelu_bwd": _gelu_bwd, "attn_fwd_lse": _attn_fwd_lse, "attn_bwd": _attn_bwd,
         "gn_bwd_mapped": _gn_bwd_mapped, "simple_tail_bwd": _simple_tail_bwd, "silu_bwd": _silu_bwd}

MUTANTS = {
    "wgrad": ("drop_chunk_last_row", "drop_partial_kstep", "no_xbound", "cross_sample", "side_column", "ldx_as_width",
              "ldy_as_width", "drop_chunk"),
    "wgrad_mapped": ("drop_chunk_last_row", "no_xbound", "cross_sample", "side_column", "drop_chunk", "map_ignored"),
    "colsum": ("drop_last_row", "ld_as_width"),
    "gn_stats": ("divisor_n",),
    "gn_bwd": ("drop_xh_term", "gelu_at_xh"),
    "gn_bwd_mapped": ("drop_xh_term", "gelu_at_xh", "padded_lane"),
    "film_bwd": ("de_no_scale", "ds_without_e"),
    "mse": ("padded_lane", "padded_n"),
    "pool_bwd": ("last_max", "assign"),
    "up_bwd": ("window_short_lo", "window_short_hi", "nin1_one_output", "assign"),
    "ln_fwd": ("no_eps", "drop_last_lane"),
    "ln_bwd": ("drop_add", "ragged_block_missing", "drop_xh_term"),
    "attn_fwd_lse": ("lse_no_max", "first256", "heads_swapped"),
    "attn_bwd": ("no_scale_dq", "drop_rowsum", "first256", "heads_swapped"),
    "mish_bwd": ("saturate_early", "drop_xpdf"),
    "silu_bwd": ("saturate_early", "drop_xpdf"),
    "gelu_bwd": ("saturate_early", "drop_xpdf"),
    "simple_tail_bwd": ("dz_pad_kept", "drop_last_row"),
}


def ref64(op, inp, mutant=None):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return {k: np.asarray(v, F64) for k, v in _IMPL[op](inp, F64, False, False, mutant).items()}


def scale64(op, inp):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return {k: np.asarray(v, F64) for k, v in _IMPL[op](inp, F64, True, False, None).items()}


def ref32(op, inp):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        out = _IMPL[op](inp, F32, False, True, None)
    for k, v in out.items():
        assert np.asarray(v).dtype == F32 or op == "pool_bwd", (op, k, np.asarray(v).dtype)
    return {k: np.asarray(v, F64) for k, v in out.items()}


def worst_ratio(got, ref, scale, tau):
    """max over every element of every output of |got - ref| / (tau S); inf where an element with bound 0 differs or is NaN."""
    worst = 0.0
    for k in ref:
        g = np.asarray(got[k], F64).reshape(ref[k].shape)
        err, bound = np.abs(g - ref[k]), tau * scale[k]
        bad = ~(err <= bound)                                                  # NaN counts as a violation
        if bad.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(bound > 0, err / bound, np.inf)
            r = np.where(np.isnan(r), np.inf, r)
            worst = max(worst, float(r[bad].max()))
        ok = ~bad & (bound > 0)
        if ok.any():
            worst = max(worst, float((err[ok] / bound[ok]).max()))
    return worst


def tau(op, inp, r64=None, s64=None, refs=None):
    """4 x the sequential float32 reference's own worst error in units of S, floored for the math-library ops.
    refs: (ref64, scale64, ref32, FLOOR_U) of another family of ops (tests/stream_ops_ref.py); None: this module's."""
    ref64, scale64, ref32, FLOOR_U = refs or (globals()[k] for k in ("ref64", "scale64", "ref32", "FLOOR_U"))
    r64 = ref64(op, inp) if r64 is None else r64
    s64 = scale64(op, inp) if s64 is None else s64
    r32 = ref32(op, inp)
    worst = 0.0
    for k in r64:
        err, s = np.abs(r32[k] - r64[k]), s64[k]
        assert np.all(err[s == 0] == 0), (op, k, "ref32 differs where S is zero")
        if (s > 0).any():
            worst = max(worst, float((err[s > 0] / s[s > 0]).max()))
    assert np.isfinite(worst), op
    t = 4.0 * worst
    if worst > 0 or op in FLOOR_U:
        t = max(t, FLOOR_U.get(op, 0) * U)
    return t


# ---- data ------------------------------------------------------------------------------------------------------------------
def _seed(op, cid):
    return zlib.crc32(f"{op}/{cid}".encode())


def _randn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(F32)


def _edges(rng, B, rows, C):
    """Per-sample mean 50 with spread 0.5; the last sample all zero (variance 0: only eps is left)."""
    v = (50 + 0.5 * rng.standard_normal((B, rows, C))).astype(F32)
    v[-1] = 0
    return v


def _edge_gain(rng, C):
    g = _randn(rng, C)
    g[::3] = -np.abs(g[::3])
    g[1::7] = 0
    return g


def _stats32(y, pos):
    """mean and rstd of the real lanes in float64, rounded to float32: what the op under test is given."""
    real = y[:, :, pos].astype(F64).reshape(y.shape[0], -1)
    mean = real.mean(1)
    var = ((real - mean[:, None]) ** 2).mean(1)
    return mean.astype(F32), (1 / np.sqrt(var + EPS)).astype(F32)


EXTREMES = np.array([s * v for v in (0.0, 1e-6, 1.0, 5.0, 19.99, 20.0, 20.01, 50.0, 88.0, 100.0, 1e4) for s in (1.0, -1.0)], F32)


def cat_map(runs, width):
    """storage lanes of a concatenation's real channels: runs of (start, count)"""
    pos = np.concatenate([np.arange(s, s + n) for s, n in runs]).astype(np.int32)
    assert pos.max() < width
    return pos


def cases(op):
    """[(case id, parameters)]: the shapes and flavours of one op."""
    C = []
    add = lambda cid, **kw: C.append((cid, kw))
    if op == "wgrad":
        base = dict(H=1, W=1, taps=1, Co=64, Ci=64, conv9=0, flavour="unit")
        add("M1409_t1", **{**base, "B": 1409, "geom": (22, 68)})
        add("M1409_t1_zero", **{**base, "B": 1409, "geom": (22, 68), "flavour": "zero"})
        add("M1409_t1_large", **{**base, "B": 1409, "geom": (22, 68), "flavour": "large"})
        add("B5_5x8_t9", **{**base, "B": 5, "H": 5, "W": 8, "taps": 9, "conv9": 1, "geom": (3, 68)})
        add("B3_8x8_t9_ci1", **{**base, "B": 3, "H": 8, "W": 8, "taps": 9, "conv9": 1, "Ci": 1, "geom": (3, 64)})
        add("B5_4x1_t3", **{**base, "B": 5, "H": 4, "W": 1, "taps": 3, "conv9": 1, "geom": (1, 20)})
        add("M3_film_linear", **{**base, "B": 3, "Co": 128, "Ci": 14, "ldx": 64, "geom": (1, 4)})
        add("M7_in_proj", **{**base, "B": 7, "Co": 192, "Ci": 64, "ldy": 200, "geom": (1, 8)})
        add("B2_13x5_t9_co128", **{**base, "B": 2, "H": 13, "W": 5, "taps": 9, "conv9": 1, "Co": 128, "geom": (2, 68)})
    elif op == "wgrad_mapped":
        maps = dict(Co=128, Ci=128, pos_o=cat_map([(0, 48), (64, 32)], 128), pos_i=cat_map([(0, 64), (96, 32)], 128))
        add("B2_6x4_t9", B=2, H=6, W=4, taps=9, geom=(1, 48), flavour="unit", **maps)
        add("B3_11x4_t9", B=3, H=11, W=4, taps=9, geom=(2, 68), flavour="unit", **maps)
        add("B5_4x1_t3", B=5, H=4, W=1, taps=3, geom=(1, 20), flavour="unit", **maps)
        add("B2_6x4_t9_zero", B=2, H=6, W=4, taps=9, geom=(1, 48), flavour="zero", **maps)
    elif op == "colsum":
        for M in (1, 255, 256, 257, 1000):
            add(f"M{M}", M=M, C=24, ld=40, off=0, flavour="unit")
        add("ln_param", M=3, C=64, ld=128, off=64, flavour="unit")             # src + C, ld = 2 C, M = the block count
        add("M257_zero", M=257, C=24, ld=40, off=0, flavour="zero")
    elif op in ("gn_stats", "gn_bwd", "gn_bwd_mapped"):
        if op == "gn_bwd_mapped" or op == "gn_stats":
            # 320 + 192 real channels fill a 512-wide storage; the gap case keeps the two runs at lanes 0 and 320
            maps = (("c128r80", 128, cat_map([(0, 80)], 128)), ("c512r320+192", 512, cat_map([(0, 320), (320, 192)], 512)),
                    ("c512r288+160gap", 512, cat_map([(0, 288), (320, 160)], 512)))
        else:
            maps = ()
        plain = () if op == "gn_bwd_mapped" else tuple((f"c{c}", c, np.arange(c, dtype=np.int32)) for c in (64, 128, 256, 512))
        for name, c, pos in plain + maps:
            for HW in (4, 5, 64):
                if op == "gn_stats":
                    add(f"{name}_hw{HW}", B=3, HW=HW, C=c, pos=pos, flavour="unit")
                    if HW != 4:
                        add(f"{name}_hw{HW}_offsets", B=3, HW=HW, C=c, pos=pos, flavour="offsets")
                    continue
                gelu = 1 if HW != 5 else 0
                add(f"{name}_hw{HW}_gelu{gelu}", B=3, HW=HW, C=c, pos=pos, gelu=gelu, flavour="unit")
                if HW == 5:
                    add(f"{name}_hw5_gelu1_offsets", B=3, HW=HW, C=c, pos=pos, gelu=1, flavour="offsets")
                if HW == 4:
                    add(f"{name}_hw4_gelu0_zero", B=3, HW=HW, C=c, pos=pos, gelu=0, flavour="zero")
    elif op == "film_bwd":
        for c in (64, 512):
            for HW in (4, 64):
                add(f"c{c}_hw{HW}_film_tB", B=3, HW=HW, C=c, T=7, t=(0, 6, 3), film=1, flavour="unit")
                add(f"c{c}_hw{HW}_nofilm_t1", B=3, HW=HW, C=c, T=7, t=(6,), film=0, flavour="unit")
        add("c64_hw4_film_t1_first", B=3, HW=4, C=64, T=7, t=(0,), film=1, flavour="unit")
        add("c64_hw4_nofilm_tB", B=3, HW=4, C=64, T=7, t=(6, 6, 0), film=0, flavour="unit")
        add("c512_hw4_film_tB_zero", B=3, HW=4, C=512, T=7, t=(6, 0, 6), film=1, flavour="zero")
    elif op == "mse":
        for B, H0, D, Hp, Wp in ((3, 31, 3, 32, 8), (2, 16, 8, 16, 8), (5, 31, 3, 32, 8)):      # 768, 256, 1280 padded lanes
            add(f"B{B}_h{H0}d{D}", B=B, H0=H0, D=D, Hp=Hp, Wp=Wp, lh=(Hp - H0) // 2, lw=(Wp - D) // 2, flavour="unit")
        add("B3_h31d3_zero", B=3, H0=31, D=3, Hp=32, Wp=8, lh=0, lw=2, flavour="zero")
        add("B3_h31d3_no_eps_out", B=3, H0=31, D=3, Hp=32, Wp=8, lh=0, lw=2, eps_out=0, flavour="unit")     # the optional output left out
    elif op == "pool_bwd":
        for H, W in ((2, 2), (8, 2), (6, 8)):
            add(f"{H}x{W}", B=3, H=H, W=W, C=64, flavour="unit")
            add(f"{H}x{W}_ties", B=3, H=H, W=W, C=64, flavour="ties")
        add("6x8_zero", B=3, H=6, W=8, C=64, flavour="zero")
    elif op == "up_bwd":
        for h, w in ((1, 1), (4, 1), (2, 2), (16, 4), (32, 4)):
            add(f"{h}x{w}", B=2, h=h, w=w, C=64, ld=128, flavour="unit")
        add("2x2_zero", B=2, h=2, w=2, C=64, ld=128, flavour="zero")
    elif op in ("mish_bwd", "silu_bwd"):
        for cd in (14, 33):
            add(f"cd{cd}", B=3, cond_dim=cd, ld=64, nblk=6, flavour="unit")
            add(f"cd{cd}_extremes", B=3, cond_dim=cd, ld=64, nblk=6, flavour="extremes")
        add("cd14_zero", B=3, cond_dim=14, ld=64, nblk=6, flavour="zero")
    elif op == "gelu_bwd":
        for n in (42, 99, 1000):
            add(f"n{n}", n=n, flavour="unit")
            add(f"n{n}_extremes", n=n, flavour="extremes")
        add("n42_zero", n=42, flavour="zero")
    elif op in ("ln_fwd", "ln_bwd"):
        for c in (64, 128, 256):
            for rows in (1, 5, 64, 65, 130):
                fl = "offsets" if rows in (5, 130) else "unit"
                if op == "ln_fwd":
                    add(f"c{c}_r{rows}_{fl}", rows=rows, C=c, flavour=fl)
                else:
                    add(f"c{c}_r{rows}_{fl}_add{int(rows != 64)}", rows=rows, C=c, add=int(rows != 64), flavour=fl)
        if op == "ln_bwd":
            add("c64_r65_zero", rows=65, C=64, add=0, flavour="zero")
    elif op in ("attn_fwd_lse", "attn_bwd"):
        for L, d in ((4, 64), (12, 64), (16, 32), (48, 32), (64, 16), (320, 16), (512, 16)):
            add(f"L{L}d{d}", B=2, L=L, C=4 * d, heads=4, flavour="unit")
            add(f"L{L}d{d}_peaked", B=2, L=L, C=4 * d, heads=4, flavour="peaked")
        if op == "attn_bwd":
            add("L12d64_zero", B=2, L=12, C=256, heads=4, flavour="zero")
    elif op == "simple_tail_bwd":
        for Co, Cr, Cz in ((128, 80, 128), (512, 320, 384)):
            for HW in (4, 5):
                add(f"co{Co}_hw{HW}", B=3, HW=HW, Co=Co, Cr=Cr, Cz=Cz, cemb_ld=64, flavour="unit")
        add("co128_hw5_zero", B=3, HW=5, Co=128, Cr=80, Cz=128, cemb_ld=64, flavour="zero")
    else:
        raise KeyError(op)
    return C


def _peaked_qkv(rng, B, L, C, heads):
    """q, k, v that make, per (sample, head), query rows i by i mod 4:
      0  one-hot: q = g k_t with g the power of two that puts the score gap to every other key at 32 or above;
      1  two keys tied for the maximum: key 1 is a bit copy of key 0 and q = g k_0;
      2  all scores equal: q = 0;
      3  one-hot under a common offset of about +1000 on every score of the row: coordinate 0 of every key is 64 and of
         the query 64 (d 16), 88 (d 32) or 125 (d 64); each product is exact in float32.
    The other d - 1 coordinates of the keys are random directions of one norm, so a key's score with itself is the largest.
    The offset sits in coordinate 0 so that the sequential float32 sum of ref32 carries it through every later addition:
    that is the worst order for this row (with the offset last, a sequential sum rounds at that magnitude once, a kernel
    that adds partial sums several times, and ref32 would not bound it)."""
    d = C // heads
    scale = 1 / math.sqrt(d)
    kk = rng.standard_normal((B, L, heads, d - 1))
    kk *= math.sqrt(d - 1) / np.linalg.norm(kk, axis=-1, keepdims=True)
    kk[:, 1] = kk[:, 0]
    q = np.zeros((B, L, heads, d))
    for i in range(L):
        kind = i % 4
        if kind == 2:
            continue
        t = 0 if kind == 1 else 2 + (i * 7) % (L - 2)
        dots = np.einsum("bhk,bjhk->bhj", kk[:, t], kk)
        own = dots[:, :, t].copy()
        dots[:, :, t] = -np.inf
        if kind == 1:
            dots[:, :, 1] = -np.inf
        g = 2.0 ** np.ceil(np.log2(32 / ((own - dots.max(-1)) * scale)))
        q[:, i, :, 1:] = g[..., None] * kk[:, t]
        if kind == 3:
            q[:, i, :, 0] = {16: 64.0, 32: 88.0, 64: 125.0}[d]
    k = np.concatenate([np.full((B, L, heads, 1), 64.0), kk], -1)
    v = rng.standard_normal((B, L, heads, d))
    return np.stack([q, k, v], 2).astype(F32).reshape(B, L, 3 * C)


def make_inputs(op, case):
    """The float32 (and integer) inputs of one case, with its parameters."""
    cid, kw = case
    rng = np.random.default_rng(_seed(op, cid))
    fl = kw["flavour"]
    inp = dict(kw)
    zero = fl == "zero"
    if op in ("wgrad", "wgrad_mapped"):
        B, H, W, Co, Ci = kw["B"], kw["H"], kw["W"], kw["Co"], kw["Ci"]
        M = B * H * W
        ldy, ldx = kw.get("ldy", Co), kw.get("ldx", Ci)
        inp.update(ldy=ldy, ldx=ldx)
        amp = 1e3 if fl == "large" else 1.0
        inp["dy"] = _randn(rng, M, ldy, scale=0.0 if zero else amp)
        inp["x"] = _randn(rng, M, ldx, scale=amp)
    elif op == "colsum":
        M, C, ld, off = kw["M"], kw["C"], kw["ld"], kw["off"]
        inp["buf"] = _randn(rng, M, ld, scale=0.0 if zero else 1.0)
    elif op in ("gn_stats", "gn_bwd", "gn_bwd_mapped"):
        B, HW, C, pos = kw["B"], kw["HW"], kw["C"], kw["pos"]
        y = _edges(rng, B, HW, C) if fl == "offsets" else _randn(rng, B, HW, C)
        real = np.zeros(C, bool)
        real[pos] = True
        y[:, :, ~real] = 0                                                     # channel-padded storage: exact zeros
        inp["y"] = y
        inp["cnt"] = 0 if real.all() else HW * int(real.sum())
        if op != "gn_stats":
            inp["mean"], inp["rstd"] = _stats32(y, pos)
            inp["gamma"] = _edge_gain(rng, C) if fl == "offsets" else (1 + 0.3 * _randn(rng, C))
            inp["beta"] = 0.3 * _randn(rng, C)
            inp["g"] = _randn(rng, B, HW, C, scale=0.0 if zero else 1.0)
    elif op == "film_bwd":
        B, HW, C, T = kw["B"], kw["HW"], kw["C"], kw["T"]
        inp["z"], inp["temb"] = _randn(rng, B, HW, C), _randn(rng, T, C)
        inp["film"] = _randn(rng, B, 2 * C) if kw["film"] else None
        inp["dout"] = _randn(rng, B, HW, C, scale=0.0 if zero else 1.0)
        inp["t"] = np.asarray(kw["t"], np.int32)
    elif op == "mse":
        inp["eps_pad"] = _randn(rng, kw["B"], kw["Hp"], kw["Wp"])
        inp["noise"] = _randn(rng, kw["B"], kw["H0"], kw["D"])
        if zero:                                                               # eps == noise: loss and gradient exactly zero
            inp["eps_pad"][:, kw["lh"]:kw["lh"] + kw["H0"], kw["lw"]:kw["lw"] + kw["D"]] = inp["noise"]
    elif op == "pool_bwd":
        B, H, W, C = kw["B"], kw["H"], kw["W"], kw["C"]
        x = _randn(rng, B, H, W, C)
        if fl == "ties":
            x = np.round(np.clip(x, -1, 1)).astype(F32)                        # {-1, 0, 1}: most windows tie
            x[0, :2, :2, :8] = 0.5                                             # all four entries equal
            x[1, :2, :2, :8] = np.array([[-0.0, 0.0], [0.0, -0.0]], F32)[:, :, None]     # -0.0 first: +0.0 is no larger
            x[2, :2, :2, :8] = np.array([[-1.0, 0.0], [-0.0, 0.0]], F32)[:, :, None]
        inp["in"] = x
        inp["dout"] = _randn(rng, B, H // 2, W // 2, C, scale=0.0 if zero else 1.0)
        inp["din"] = _randn(rng, B, H, W, C)
    elif op == "up_bwd":
        B, h, w, C, ld = kw["B"], kw["h"], kw["w"], kw["C"], kw["ld"]
        inp["dcat"] = _randn(rng, B * 4 * h * w, ld)
        if zero:
            inp["dcat"][:, :C] = 0
        inp["dx"] = _randn(rng, B, h, w, C)
    elif op in ("mish_bwd", "silu_bwd", "gelu_bwd"):
        if op == "gelu_bwd":
            shape = (kw["n"],)
        else:
            shape = (kw["B"], kw["cond_dim"])
        x = _randn(rng, *shape)
        if fl == "extremes":
            flat = x.reshape(-1)
            flat[:min(len(EXTREMES), flat.size)] = EXTREMES[:flat.size]
            flat[len(EXTREMES):] *= 8
        sc = 0.0 if zero else 1.0
        if op == "mish_bwd":
            inp["cond"], inp["dm"] = x, _randn(rng, kw["nblk"], kw["B"], kw["ld"], scale=sc)
        elif op == "silu_bwd":
            inp["cond"], inp["ds"] = x, _randn(rng, kw["B"], kw["ld"], scale=sc)
        else:
            inp["u"], inp["dh"] = x, _randn(rng, kw["n"], scale=sc)
    elif op in ("ln_fwd", "ln_bwd"):
        rows, C = kw["rows"], kw["C"]
        x = _edges(rng, 1, rows, C)[0] if fl == "offsets" else _randn(rng, rows, C)
        if fl == "offsets" and rows > 1:
            x[-1] = 0
            x[0] = 50 + 0.5 * rng.standard_normal(C).astype(F32)
        inp["x"] = x
        g = _edge_gain(rng, C) if fl == "offsets" else (1 + 0.3 * _randn(rng, C))
        if op == "ln_fwd":
            inp["g"], inp["b"] = g, 0.3 * _randn(rng, C)
        else:
            x64 = x.astype(F64)
            mean = x64.mean(1)
            inp["mean"] = mean.astype(F32)
            inp["rstd"] = (1 / np.sqrt(((x64 - mean[:, None]) ** 2).mean(1) + EPS)).astype(F32)
            inp["gamma"] = g
            inp["gy"] = _randn(rng, rows, C, scale=0.0 if zero else 1.0)
            inp["add"] = _randn(rng, rows, C) if kw["add"] else None
    elif op in ("attn_fwd_lse", "attn_bwd"):
        B, L, C, heads = kw["B"], kw["L"], kw["C"], kw["heads"]
        inp["qkv"] = _peaked_qkv(rng, B, L, C, heads) if fl == "peaked" else _randn(rng, B, L, 3 * C)
        if op == "attn_bwd":
            f = ref64("attn_fwd_lse", inp)
            inp["out"], inp["lse"] = f["out"].astype(F32), f["lse"].astype(F32)
            do = _randn(rng, B, L, C, scale=0.0 if zero else 1.0)
            if fl == "peaked":                                                 # dO aligned with O (even rows), orthogonal to O (odd rows)
                d = C // heads
                o = inp["out"].reshape(B, L, heads, d)
                r = do.reshape(B, L, heads, d)
                proj = (r * o).sum(-1, keepdims=True) / np.maximum((o * o).sum(-1, keepdims=True), 1e-30)
                do = np.where((np.arange(L) % 2 == 0)[None, :, None, None], 3 * o, r - proj * o).astype(F32).reshape(B, L, C)
            inp["dout"] = do
    elif op == "simple_tail_bwd":
        inp["dout"] = _randn(rng, kw["B"], kw["HW"], kw["Co"], scale=0.0 if zero else 1.0)
    else:
        raise KeyError(op)
    return inp


# ---- the launch of one case through spdm_op_train (include/spdm.h) ------------------------------------------------------------
def launch_plan(op, inp):
    """(dims, buffers, index arrays, outputs) of one case as the hook takes them.  buffers: ("in" | "inout", float32 array),
    ("out", elements) or None (an optional buffer left out); outputs: {name: (buffer index, shape, row stride or None)}."""
    g = lambda *names: [int(inp[n]) for n in names]
    I, O = (lambda a: ("in", np.ascontiguousarray(a, F32))), (lambda n: ("out", int(n)))
    # rows of ld floats of which the last is `width` long: exactly the extent the launch reads
    S = lambda a, ld, width: ("in", np.ascontiguousarray(a, F32).reshape(-1, ld).ravel()[:a.size - ld + width])
    idx = []
    if op == "wgrad":
        dims = g("B", "H", "W", "taps", "Co", "Ci", "conv9", "ldy", "ldx")
        shape = (inp["Co"], inp["Ci"], 3, 3) if inp["conv9"] else (inp["Co"], inp["Ci"])
        bufs = [S(inp["dy"], inp["ldy"], inp["Co"]), S(inp["x"], inp["ldx"], inp["Ci"]), O(np.prod(shape))]
        outs = {"dst": (2, shape, None)}
    elif op == "wgrad_mapped":
        no, ni = len(inp["pos_o"]), len(inp["pos_i"])
        dims = g("B", "H", "W", "taps", "Co", "Ci") + [no, ni]
        bufs, outs = [I(inp["dy"]), I(inp["x"]), O(no * ni * 9)], {"dst": (2, (no, ni, 3, 3), None)}
        idx = [inp["pos_o"], inp["pos_i"]]
    elif op == "colsum":
        dims = g("M", "C", "ld")
        src = inp["buf"].ravel()[inp["off"]:inp["off"] + (inp["M"] - 1) * inp["ld"] + inp["C"]]
        bufs, outs = [I(src), O(inp["C"])], {"dst": (1, (inp["C"],), None)}
    elif op == "gn_stats":
        B, HW, C = inp["y"].shape
        dims = [B, HW * C, int(inp["cnt"])]
        bufs, outs = [I(inp["y"]), O(B), O(B)], {"mean": (1, (B,), None), "rstd": (2, (B,), None)}
    elif op in ("gn_bwd", "gn_bwd_mapped"):
        B, HW, C = inp["y"].shape
        dims = [B, HW, C, int(inp["gelu"])]
        if op == "gn_bwd_mapped":
            dims.append(len(inp["pos"]))
            idx = [inp["pos"]]
        bufs = [I(inp[k]) for k in ("y", "mean", "rstd", "gamma", "beta", "g")] + [O(B * HW * C), O(B * C * 2)]
        outs = {"dy": (6, (B, HW, C), None), "dgb": (7, (B, C, 2), None)}
    elif op == "film_bwd":
        B, HW, C = inp["z"].shape
        film = inp["film"] is not None
        dims = [B, HW, C, len(inp["t"]), int(inp["T"])]
        bufs = [I(inp["z"]), I(inp["temb"]), I(inp["film"]) if film else None, I(inp["dout"]), O(B * HW * C), O(B * C),
                O(B * 2 * C) if film else None]
        outs = {"dz": (4, (B, HW, C), None), "de": (5, (B, C), None)}
        if film:
            outs["dfilm"] = (6, (B, 2 * C), None)
        idx = [inp["t"]]
    elif op == "mse":
        dims = g("B", "H0", "D", "Hp", "Wp", "lh", "lw")
        B, H0, D, Hp, Wp = dims[:5]
        bufs = [I(inp["eps_pad"]), I(inp["noise"]), O(1), O(B * Hp * Wp), O(B * H0 * D)]
        outs = {"loss": (2, (1,), None), "deps_pad": (3, (B, Hp, Wp), None), "eps_out": (4, (B, H0, D), None)}
        if not inp.get("eps_out", 1):
            bufs[4] = None
            del outs["eps_out"]
    elif op == "pool_bwd":
        dims = g("B", "H", "W", "C")
        bufs, outs = [I(inp["in"]), I(inp["dout"]), ("inout", inp["din"])], {"din": (2, inp["din"].shape, None)}
    elif op == "up_bwd":
        dims = g("B", "h", "w", "C", "ld")
        bufs, outs = [S(inp["dcat"], inp["ld"], inp["C"]), ("inout", inp["dx"])], {"dx": (1, inp["dx"].shape, None)}
    elif op == "mish_bwd":
        dims = g("nblk", "B", "ld", "cond_dim")
        n = inp["B"] * inp["cond_dim"]
        bufs, outs = [S(inp["dm"], inp["ld"], inp["cond_dim"]), I(inp["cond"]), O(n)], {"grad_cond": (2, inp["cond"].shape, None)}
    elif op == "silu_bwd":
        dims = g("B", "cond_dim", "ld")
        bufs = [S(inp["ds"], inp["ld"], inp["cond_dim"]), I(inp["cond"]), O(inp["B"] * inp["cond_dim"])]
        outs = {"grad_cond": (2, inp["cond"].shape, None)}
    elif op == "gelu_bwd":
        dims = g("n")
        bufs, outs = [I(inp["u"]), I(inp["dh"]), O(inp["n"])], {"du": (2, (inp["n"],), None)}
    elif op == "ln_fwd":
        rows, C = dims = g("rows", "C")
        bufs = [I(inp["x"]), I(inp["g"]), I(inp["b"]), O(rows * C), O(rows), O(rows)]
        outs = {"y": (3, (rows, C), None), "mean": (4, (rows,), None), "rstd": (5, (rows,), None)}
    elif op == "ln_bwd":
        rows, C = dims = g("rows", "C")
        nb = ln_bwd_blocks(rows)
        bufs = [I(inp[k]) for k in ("x", "mean", "rstd", "gamma", "gy")] + [I(inp["add"]) if inp["add"] is not None else None,
                                                                           O(rows * C), O(nb * 2 * C)]
        outs = {"dx": (6, (rows, C), None), "part": (7, (nb, 2 * C), None)}
    elif op in ("attn_fwd_lse", "attn_bwd"):
        B, L, C, heads = dims = g("B", "L", "C", "heads")
        if op == "attn_fwd_lse":
            bufs = [I(inp["qkv"]), O(B * L * C), O(B * heads * L)]
            outs = {"out": (1, (B, L, C), None), "lse": (2, (B, heads, L), None)}
        else:
            bufs = [I(inp[k]) for k in ("qkv", "out", "dout", "lse")] + [O(B * L * 3 * C)]
            outs = {"dqkv": (4, (B, L, 3 * C), None)}
    elif op == "simple_tail_bwd":
        B, HW, Co, Cr, Cz, ld = dims = g("B", "HW", "Co", "Cr", "Cz", "cemb_ld")
        bufs = [I(inp["dout"]), O(B * HW * Cz), O(B * Cr), O((B - 1) * ld + 32)]
        outs = {"dz": (1, (B, HW, Cz), None), "dtemb": (2, (B, Cr), None), "dcemb": (3, (B, 32), ld)}
    else:
        raise KeyError(op)
    return dims, bufs, [np.ascontiguousarray(a, np.int32) for a in idx], outs


def expected_info(op, inp):
    """info[] the hook reports: (chunks, rows per chunk) of a weight gradient, the block count of ln_bwd; None otherwise."""
    if op in ("wgrad", "wgrad_mapped"):
        return wgrad_geometry(inp["B"] * inp["H"] * inp["W"], inp["taps"], inp["Co"], inp["Ci"])
    if op == "ln_bwd":
        return (ln_bwd_blocks(inp["rows"]),)
    return None
