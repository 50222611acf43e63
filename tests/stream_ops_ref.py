"""Plain CPU references of ONE streaming launch of the forward / sampling path (spdm_op_stream, include/spdm.h), for tests only:
numpy (torch for erf), nothing from the project.  The contract is tests/train_ops_ref.py's, whose helpers this module imports:

  ref64(op, inp)      the operation in float64, written from its definition in the reference project's modules, on the float32
                      values the kernel is given (every comparison -- the pooling maximum -- is then exact);
  scale64(op, inp)    the same expression with every term in absolute value, (v - mu) counting |v| + |mu|: the S of the tolerance;
  ref32(op, inp)      the same formulas in float32 with every sum taken SEQUENTIALLY in float32;
  MUTANTS[op]         float64 models of the mistakes the kernel could make (ref64(op, inp, mutant=name)).

Tolerance, per element: |got - ref64| <= TAU * S, TAU = 4 * max |ref32 - ref64| / S from the references alone (tau()), floored by
FLOOR_U[op] * u for the ops with math-library calls.  Where S is zero the element must be equal: padded lanes, copied channels,
zero-padded columns, a MaxPool with no GroupNorm, the step and t words, outputs that no data reaches.

A pending GroupNorm(1, C) is given as the kernels get it: float64 partial sums {sum x, sum x^2} per (sample, producer tile), which
make_inputs computes from the case's own tensor and splits over exactly the slots the consumer reads; every other slot is NaN.
ref64 evaluates mean, the clamped variance and rstd = 1 / sqrt(var + 1e-5) from them in float64.

The GELU of the concat-conditioned U-Net is device_utils.h's one-exponential form v Phi(v) = max(v, 0) - |v| 2^E(min(|v|, 6)), a
degree-6 fit whose error is ABSOLUTE (documented there: 2.6e-7 float32-emulated, 6e-7 held on the device by tests/test_gpu_ops.py),
not relative to |v|: at v -> 0 it is 6e-6 |v|.  S of a GELU output therefore counts 1 (the range of Phi) beside |v|, and the
floor carries GELU_ABS_U = 6e-7 / u: TAU S >= 6e-7 (1 + |v|).

out_step's scheduler update is not approximated at all: step_f32 restates the kernel's documented operation order in float32,
every mul / sub / div / add rounded by itself (numpy has no FMA), and the expected x, history and in-painted rows are those
values with S = 0 -- bit for bit.  From the features, the restatement is applied to the eps the launch's own eps-only mode
stored (inp["eps_dev"], set by the GPU test; on the CPU the float64 eps rounded once stands in).  Only eps itself and the
Philox normal (logf, sinf, cosf) carry a bound.

cases(op) is the case table the CPU and GPU tests share; make_inputs(op, case) the data; launch_plan(op, inp) the hook's arguments.
"""
import math

import numpy as np
import torch

import train_ops_ref as T
from train_ops_ref import EPS, EXTREMES, F32, F64, TINY, U, _edge_gain, _erf, _randn, _seed, ssum, worst_ratio  # noqa: F401

OPS = ("conv_in", "pool", "upcat", "film_apply", "film_coef", "layernorm", "mish_pad", "silu_pad", "silu", "dc_finish",
       "simple_tail", "splitk_combine", "out_step")
GN_CONSUMERS = ("pool", "upcat", "film_apply", "film_coef", "dc_finish", "simple_tail")

GELU_ABS_U = math.ceil(6e-7 / U)     # gelu_erf's documented absolute error (device_utils.h), in units of u: 11
# Floors of TAU in units of u: roundings on the longest dependency chain of one element (1 u each) plus the documented bounds of
# the device functions on it (HIP math API: expf 1 ulp, tanhf 2, log1pf 1; v_exp_f32 1; division and sqrtf correctly rounded;
# k ulp = 2 k u).  A pending GroupNorm adds: mean and rstd rounded to float32 (2), rstd * gamma (1), v - mu (1), * sc (1), + beta (1).
FLOOR_U = {
    # expf (2), log1pf (2) amplified by at most 1 through tanh, tanhf (4), x * (1)
    "mish_pad": 9,
    # expf (2), 1 + (1), x / (1)
    "silu_pad": 4, "silu": 4,
    # GroupNorm (6), + res (1); gelu_erf: 6 fma (6) on an exponent of at most 30 -- 2^E's relative error is ln 2 |E| u per rounding,
    # but E is that large only where 2^E < 2^-20, so the absolute error stays below u; v_exp_f32 (2), the last fma (1);
    # the fit itself: GELU_ABS_U on the 1 in S
    "dc_finish": 16 + GELU_ABS_U,
    # the same and + temb (1)
    "simple_tail": 17 + GELU_ABS_U,
    # mean: * 1 / C (1); d = v - mean (1), d d (1), * 1 / C (1), + eps (1), sqrtf (1), 1 / (1), * rstd (1), * g (1), + b (1)
    "layernorm": 10,
    # the Philox normal (the only part of a scheduler step that is not restated bit for bit) and the outc dot product:
    # logf (2), sqrtf (1), 2 pi u2 (1: the angle's rounding, which S carries amplified by the radius), sinf / cosf (4), r * (1),
    # c5 * (1), prev + (1)
    "out_step": 11,
}
SQRT_HALF = math.sqrt(0.5)


# ---- a pending GroupNorm ----------------------------------------------------------------------------------------------------
def gn_reads(B, HW, m_tile, n_tiles):
    """slots the consumer adds for each sample: the tiles its rows touch, n_tiles each (sample_mean_rstd_wave)"""
    return [((b * HW + HW - 1) // m_tile - (b * HW) // m_tile + 1) * n_tiles for b in range(B)]


def gn_geometry(kind, HW):
    """(m_tile, n_tiles) of a producer whose partials put the consumer on one of its summation paths"""
    if kind == "serial":                   # at most 8 slots: one thread adds them in order
        return HW, 2
    if kind == "mid":                      # 9 .. 64 slots: one per lane
        return max(1, HW // 4), 4 if HW >= 4 else 12
    if kind == "wide":                     # more than 64: lane i adds slots i, i + 64, ...
        return 1, -(-65 // HW)
    if kind == "straddle":                 # m_tile does not divide HW: tiles straddle samples, first = b HW / m_tile matters
        return HW // 2 + 1, 5
    if kind == "straddle_serial":          # the same on the serial path
        return HW // 2 + 1, 2
    raise KeyError(kind)


def make_partials(x, m_tile, n_tiles, spare=1):
    """[B][slots][2] float64 {sum, sum of squares} of x [B][HW][C] per (sample, row tile, channel tile), in the slot the consumer
    reads it from; unused slots NaN."""
    B, HW, C = x.shape
    reads = gn_reads(B, HW, m_tile, n_tiles)
    out = np.full((B, max(reads) + spare, 2), np.nan, F64)
    x64 = x.astype(F64)
    chans = np.array_split(np.arange(C), n_tiles)
    for b in range(B):
        first = (b * HW) // m_tile
        for i in range(reads[b] // n_tiles):
            r0, r1 = max((first + i) * m_tile - b * HW, 0), min((first + i + 1) * m_tile - b * HW, HW)
            for nt, ch in enumerate(chans):
                v = x64[b, r0:r1][:, ch]
                out[b, i * n_tiles + nt] = (v.sum(), (v * v).sum())
    return out


def _gn_stats(g, dt, mutant):
    """(mean [B], rstd [B]) in dt from the partials, as the kernels evaluate them: float64 sums, E[x^2] - mean^2 clamped at 0,
    then rounded to the consumer's float32 (dt float32 only)."""
    if g is None:
        return None
    st, HW, C = g["stats"], g["HW"], g["C"]
    B = st.shape[0]
    reads = gn_reads(B, HW, g["m_tile"], g["n_tiles"])
    cn = C if mutant == "cnorm_as_C" else g["cnorm"]
    mu, rs = np.zeros(B, F64), np.zeros(B, F64)
    for b in range(B):
        n = reads[b] - (1 if mutant == "slot_short_by_one" else 0)
        p = st[0 if mutant == "cross_sample_slots" else b, :n]
        m = p[:, 0].sum() / (cn * HW)
        var = p[:, 1].sum() / (cn * HW) - m * m
        if var < 0 and mutant != "no_var_clamp":
            var = 0.0
        mu[b], rs[b] = m, 1 / np.sqrt(var + EPS)
    return mu.astype(dt), rs.astype(dt)


def _affine(x, st, g, dt, ab):
    """GN(x) = (x - mu) (rstd gamma) + beta on x [B][rows][C'] (C' leading channels of gamma / beta), or x when none pends"""
    if st is None:
        return np.abs(x) if ab else x
    mu, rs = (v[:, None, None] for v in st)
    n = x.shape[2]
    ga, be = g["gamma"][:n].astype(dt), g["beta"][:n].astype(dt)
    if ab:
        return (np.abs(x) + np.abs(mu)) * (rs * np.abs(ga)) + np.abs(be)
    return (x - mu) * (rs * ga) + be


# ---- the ops: f(inp, dt, ab, seq, mutant) -> {name: array} --------------------------------------------------------------------
def conv_in_parts(HW, B):
    return 4 if B < 1024 and HW % 64 == 0 else 1


def stats_slots(HW, m_tile, n_tiles):
    return ((HW + m_tile - 2) // m_tile + 1) * n_tiles


def combine_rows(HW, N):
    r = HW
    while r % 2 == 0 and r * N > 2048:
        r //= 2
    return r


def _conv_in(inp, dt, ab, seq, mutant):
    """Conv2d(1, 64, 3, padding=1, bias=False) of the (H0, D) trajectory zero-padded to (Hp, Wp) at (lh, lw); the GroupNorm partial
    sums of its output per row part; the loop bookkeeping step <- adv (or step0 + 1), t <- timesteps[clamp(step)]."""
    B, H0, D, Hp, Wp, lh, lw = (inp[k] for k in ("B", "H0", "D", "Hp", "Wp", "lh", "lw"))
    x, w = inp["x"].astype(dt), inp["w"].astype(dt)
    if ab:
        x, w = np.abs(x), np.abs(w)
    if mutant == "pad_offset_ignored":
        lh = lw = 0
    img = np.zeros((B, Hp, Wp), dt)
    img[:, lh:lh + H0, lw:lw + D] = x
    HW = Hp * Wp
    y = np.zeros((B, HW, 64), dt)
    flat = img.reshape(B, HW)
    hh, ww = np.divmod(np.arange(HW), Wp)
    for t in range(9):
        ys, xs = hh + t // 3 - 1, ww + t % 3 - 1
        ok = (ys >= 0) & (ys < Hp) & (xs >= 0) & (xs < Wp)
        src = ys * Wp + xs
        if mutant == "no_zero_pad":        # no column bound: the tap wraps into the neighbouring row
            ok = (src >= 0) & (src < HW)
        tap = np.where(ok[None, :], flat[:, np.clip(src, 0, HW - 1)], 0).astype(dt)
        y = y + tap[:, :, None] * w[t][None, None, :]
    parts = inp["parts"]
    rp = HW // parts
    yp = y.reshape(B, parts, rp * 64)
    if mutant == "part_dropped":           # the last 16-row pass of every part never reaches the sums
        yp = yp[:, :, :(rp - 16) * 64]
    stats = np.stack([ssum(yp, 2, seq), ssum(yp * yp, 2, seq)], axis=2)
    out = {"dst": y, "stats": stats}
    if inp["adv"] >= -1:
        step = inp["adv"] if inp["adv"] >= 0 else inp["step0"] + 1
        t = int(inp["timesteps"][min(max(step, 0), inp["n_steps"] - 1)])
        out["words"] = np.zeros(2, dt) if ab else np.array([step, t], dt)
    return out


def _pool(inp, dt, ab, seq, mutant):
    """MaxPool2d(2) of GN(x): the maximum over the four taps of the affine (max does not commute with a negative gain)."""
    B, H, W, C = (inp[k] for k in ("B", "H", "W", "C"))
    x = inp["x"].astype(dt)
    st = _gn_stats(inp["gn"], dt, mutant)
    win = lambda a: a.reshape(B, H // 2, 2, W // 2, 2, C)
    if mutant == "affine_after_max":
        a = _affine(win(x).max(axis=(2, 4)).reshape(B, -1, C), st, inp["gn"], dt, ab)
        return {"dst": a}
    a = win(_affine(x, st, inp["gn"], dt, ab))
    if mutant == "drop_odd_column":
        a = a[:, :, :, :, :1]
    y = a.max(axis=(2, 4)).reshape(B, -1, C)
    if ab and st is None:
        y = np.zeros_like(y)               # a maximum of the given values: equality
    return {"dst": y}


def _up_axis(n_in, dt, mutant):
    """(i0, i1, l0, l1) of nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) along one axis"""
    n_out = 2 * n_in
    o = np.arange(n_out).astype(dt)
    if mutant == "align_corners_false":
        src = np.maximum((o + dt(0.5)) / dt(2) - dt(0.5), 0).astype(dt)
    else:
        sc = dt(n_in - 1) / dt(n_out - 1)
        src = (sc * o).astype(dt)
    i0 = np.floor(src).astype(np.int64)
    i1 = i0 + 1 if mutant == "no_edge_clamp" else i0 + (i0 < n_in - 1)
    l1 = np.clip(src - i0.astype(dt), 0, 1).astype(dt)
    return i0, i1, (dt(1) - l1).astype(dt), l1


def _upcat(inp, dt, ab, seq, mutant):
    """cat([bilinear x2 (align_corners=True) of GN(up), GN(skip)], channels)."""
    B, Hin, Win, Cu, Cs = (inp[k] for k in ("B", "Hin", "Win", "Cu", "Cs"))
    st_u = _gn_stats(inp["gn"], dt, mutant)
    a = _affine(inp["up"].astype(dt), st_u, inp["gn"], dt, ab).reshape(B * Hin * Win, Cu)
    a = np.concatenate([a, np.full((Win + 2, Cu), np.nan, dt)])               # what lies beyond the tensor is unknown
    h0, h1, lh0, lh1 = _up_axis(Hin, dt, mutant)
    w0, w1, lw0, lw1 = _up_axis(Win, dt, mutant)
    at = lambda hs, ws: a[((np.arange(B)[:, None, None] * Hin + hs[None, :, None]) * Win + ws[None, None, :])]
    L = lambda v: v[None, :, None, None]
    Lw = lambda v: v[None, None, :, None]
    y = L(lh0) * (Lw(lw0) * at(h0, w0) + Lw(lw1) * at(h0, w1)) + L(lh1) * (Lw(lw0) * at(h1, w0) + Lw(lw1) * at(h1, w1))
    y = y.reshape(B, 4 * Hin * Win, Cu).astype(dt)
    if Cs == 0:
        return {"dst": y}
    g_s = inp["gn_skip"]
    st_s = _gn_stats(g_s, dt, mutant)
    if mutant == "skip_stats_from_up" and st_s is not None and st_u is not None:
        st_s = st_u
    s = _affine(inp["skip"].astype(dt), st_s, g_s, dt, ab)
    if ab and st_s is None:
        s = np.zeros_like(s)               # a copy: equality
    return {"dst": np.concatenate([s, y] if mutant == "concat_swapped" else [y, s], axis=2)}


def _film_parts(inp, dt, ab, mutant):
    B, C = inp["B"], inp["C"]
    e = fs = fb = None
    if inp["temb"] is not None:
        t = np.asarray(inp["t"])
        t = np.repeat(t, B) if len(t) == 1 else t
        if mutant == "t_of_sample0":
            t = np.repeat(t[:1], B)
        e = inp["temb"].astype(dt)[t]
    if inp["film"] is not None:
        f = inp["film"].astype(dt)
        fs, fb = f[:, :C], f[:, C:]
    if ab:
        e, fs, fb = (None if v is None else np.abs(v) for v in (e, fs, fb))
    return e, fs, fb


def _film_apply(inp, dt, ab, seq, mutant):
    """y = scale (GN(x) + emb_t) + bias; row statistics {sum_c y, sum_c y^2} of every token row."""
    e, fs, fb = _film_parts(inp, dt, ab, mutant)
    st = _gn_stats(inp["gn"], dt, mutant)
    v = _affine(inp["x"].astype(dt), st, inp["gn"], dt, ab)
    pre = v if e is None else v + e[:, None, :]
    if mutant == "temb_after_scale" and e is not None and fs is not None:
        y = fs[:, None, :] * v + e[:, None, :] + fb[:, None, :]
    else:
        y = pre if fs is None else fs[:, None, :] * pre + fb[:, None, :]
    y = y.astype(dt)
    out = {"dst": y}
    if inp["row_stats"]:
        r = pre.astype(dt) if mutant == "row_stats_pre_film" else y
        out["row_stats"] = np.stack([ssum(r, 2, seq), ssum(r * r, 2, seq)], axis=2)
    return out


def _film_coef(inp, dt, ab, seq, mutant):
    """The same tail as coefficients of the raw tensor: A = scale rstd gamma, B = scale (beta - mean rstd gamma + emb_t) + bias."""
    B, C = inp["B"], inp["C"]
    e, fs, fb = _film_parts(inp, dt, ab, mutant)
    st = _gn_stats(inp["gn"], dt, mutant)
    sc, be = np.ones((B, C), dt), np.zeros((B, C), dt)
    if st is not None:
        mu, rs = (v[:, None] for v in st)
        ga, bt = inp["gn"]["gamma"].astype(dt)[None, :], inp["gn"]["beta"].astype(dt)[None, :]
        if ab:
            sc = rs * np.abs(ga)
            be = np.abs(bt) + np.abs(mu) * sc
        else:
            sc = rs * ga
            be = np.broadcast_to(bt, (B, C)) if mutant == "mean_not_folded" else bt - mu * sc
    if e is not None:
        be = be + e
    if mutant == "temb_after_scale" and e is not None and fs is not None:
        return {"ab": np.concatenate([fs * sc, fs * (be - e) + e + fb], axis=1).astype(dt)}
    if fs is None:
        return {"ab": np.concatenate([sc, be], axis=1).astype(dt)}
    return {"ab": np.concatenate([fs * sc, fs * be + fb], axis=1).astype(dt)}


def _layernorm(inp, dt, ab, seq, mutant):
    """nn.LayerNorm([C]) of every row, two-pass variance."""
    if mutant == "one_pass_variance":
        # E[x^2] - mean^2 with float32 sums, which the two-pass form is there to avoid.  Under an S that counts |x| + |mean| a
        # variance off by a few roundings of mean^2 is within the bound by construction; what the bound does see is the variance
        # of a constant row coming out below -eps (the two-pass form needs no clamp and has none).
        x = inp["x"].astype(F32)
        C = x.shape[1]
        mean = ssum(x, 1, True) / F32(C)
        var = ssum(x * x, 1, True) / F32(C) - mean * mean
        rstd = (1 / np.sqrt(var.astype(F64) + EPS))
        return {"y": (x.astype(F64) - mean[:, None]) * rstd[:, None] * inp["g"].astype(F64) + inp["b"].astype(F64)}
    return {"y": T._ln_fwd(inp, dt, ab, seq, mutant)["y"]}


def _mish(x, dt, ab, mutant):
    sat = (x >= 1) if mutant == "saturate_early" else (x > 20)         # nn.Mish's softplus threshold is 20
    with np.errstate(over="ignore"):
        sp = np.where(sat, x, np.log1p(np.exp(np.minimum(x, 80)))).astype(dt)
    th = np.tanh(sp).astype(dt)
    return (np.abs(x) * (th + TINY)) if ab else x * th


def _silu(x, dt, ab, mutant):
    sg = T._sigmoid(x)
    if mutant == "saturate_early":
        sg = np.where(x > 2, 1.0, sg).astype(dt)
    return (np.abs(x) * (sg + TINY)) if ab else (x * sg).astype(dt)


def _padded(f):
    def op(inp, dt, ab, seq, mutant):
        """dst [B][Kp] = f(cond [B][cond_dim]), zeros in the padding columns."""
        B, cd, Kp = inp["B"], inp["cond_dim"], inp["Kp"]
        x = inp["cond"].astype(dt)
        out = np.zeros((B, Kp), dt)
        if mutant == "kp_as_stride":       # the flat output index read as a flat input index
            flat = np.full(B * Kp, np.nan, dt)
            flat[:B * cd] = x.reshape(-1)
            return {"dst": f(flat, dt, ab, None).reshape(B, Kp)}
        out[:, :cd] = f(x, dt, ab, mutant)
        return {"dst": out}
    return op


def _silu_flat(inp, dt, ab, seq, mutant):
    y = _silu(inp["x"].astype(dt), dt, ab, mutant)
    if mutant == "drop_last_block":
        y = y.copy()
        y[len(y) // 256 * 256:] = np.nan
    return {"y": y}


def _gelu(v, dt, ab, mutant=None):
    """v Phi(v); ab: v is S of the argument already, and the output counts 1 for the fit's absolute error (module docstring)"""
    if ab:
        return v + 1
    if mutant == "gelu_tanh":
        return 0.5 * v * (1 + np.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))
    return (dt(0.5) * v * (1 + _erf(v * dt(SQRT_HALF)))).astype(dt)


def _dc_finish(inp, dt, ab, seq, mutant):
    """y = GELU(GN(x) + res)."""
    st = _gn_stats(inp["gn"], dt, mutant)
    v = _affine(inp["x"].astype(dt), st, inp["gn"], dt, ab)
    r = None if inp["res"] is None else (np.abs(inp["res"]) if ab else inp["res"]).astype(dt)
    if r is not None and mutant == "res_after_gelu":
        return {"dst": _gelu(v, dt, ab) + r}
    return {"dst": _gelu(v if r is None else v + r, dt, ab, mutant)}


def _simple_tail(inp, dt, ab, seq, mutant):
    """y[:, :Cr] = GELU(GN(x[:, :Cr])) + temb[t]; y[:, Cr:Cr + 32] = cemb[b]; zeros up to Co."""
    B, HW, Co, Cr = (inp[k] for k in ("B", "HW", "Co", "Cr"))
    st = _gn_stats(inp["gn"], dt, mutant)
    v = _affine(inp["x"].astype(dt)[:, :, :Cr], st, inp["gn"], dt, ab)
    t = np.asarray(inp["t"])
    t = np.repeat(t, B) if len(t) == 1 else t
    if mutant == "t_of_sample0":
        t = np.repeat(t[:1], B)
    e = inp["temb"].astype(dt)[t][:, None, :Cr]
    if ab:
        e = np.abs(e)
    y = np.zeros((B, HW, Co), dt)
    y[:, :, :Cr] = _gelu(v + e, dt, ab) if mutant == "gelu_after_temb" else _gelu(v, dt, ab) + e
    if not ab:
        y[:, :, Cr:Cr + 32] = inp["cemb"].astype(dt)[:, None, :32]
    if mutant == "pad_kept":               # the storage padding is not written
        y[:, :, Cr + 32:] = np.nan
    return {"dst": y}


def _splitk_combine(inp, dt, ab, seq, mutant):
    """dst = sum of the ksplit slabs (ascending); {sum, sum of squares} of dst per block of `rows` rows of a sample."""
    B, HW, N, ks = (inp[k] for k in ("B", "HW", "N", "ksplit"))
    p = inp["partial"].astype(dt)
    if ab:
        p = np.abs(p)
    if mutant == "drop_last_slab":
        p = p[:-1]
    elif mutant == "drop_remainder_slab":  # the slabs after the last full group of four
        p = p[:1 + (ks - 1) // 4 * 4]
    y = ssum(np.moveaxis(p, 0, -1), -1, seq).astype(dt)
    rows = combine_rows(HW, N)
    yb = y.reshape(B, HW // rows, rows * N)
    if mutant == "stats_first_pass_only":  # the first 256 x 8 float4 pieces of a block only
        yb = yb[:, :, :8192]
    return {"dst": y, "stats": np.stack([ssum(yb, 2, seq), ssum(yb * yb, 2, seq)], axis=2)}


# ---- the step kernel: outc + unpad + scheduler step + in-painting ------------------------------------------------------------
def coef_table(kind, T_, n):
    """((n, 6) float32 [sqrt(1 - abar_t), sqrt(abar_t), k_x0, k_x, k_eps, k_noise] per loop iteration, timesteps) in the operation
    order of diffusers 0.17.1's DDPMScheduler (kind 0) / DDIMScheduler (kind 1): linear betas 1e-4 .. 0.02, fixed_small variance,
    eta = 0, float32 torch scalars."""
    acp = torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, T_, dtype=torch.float32), dim=0)
    ratio = T_ // n
    ts = [int(t) for t in (np.arange(n) * ratio)[::-1]]
    rows, zero = [], torch.tensor(0.0)
    for t in ts:
        a_t = acp[t]
        a_prev = acp[t - ratio] if t - ratio >= 0 else torch.tensor(1.0)
        b_t = 1 - a_t
        if kind == 0:
            cur_a = a_t / a_prev
            cur_b = 1 - cur_a
            k_noise = torch.clamp((1 - a_prev) / (1 - a_t) * cur_b, min=1e-20) ** 0.5 if t > 0 else zero
            rows.append([b_t ** 0.5, a_t ** 0.5, (a_prev ** 0.5 * cur_b) / b_t, cur_a ** 0.5 * (1 - a_prev) / b_t, zero, k_noise])
        else:
            rows.append([b_t ** 0.5, a_t ** 0.5, a_prev ** 0.5, zero, (1 - a_prev - zero ** 2) ** 0.5, zero])
    return np.array([[float(v) for v in r] for r in rows], F32), ts


def step_f32(kind, c, x, eps, z=None):
    """The scheduler update in float32 in the kernel's documented operation order -- individually rounded mul, sub, div, add,
    never an FMA (numpy rounds every elementwise operation).  c: one float32 row of the coefficient table."""
    c, x, eps = np.asarray(c, F32), np.asarray(x, F32), np.asarray(eps, F32)
    x0 = (x - c[0] * eps) / c[1]
    if kind == 1:
        return c[2] * x0 + c[4] * eps
    prev = c[2] * x0 + c[3] * x
    if c[5] != 0 and z is not None:
        prev = prev + c[5] * np.asarray(z, F32)
    return prev


TWO_PI_F32 = F32(6.283185307179586)


def _philox_uniforms(seed, first, B, step, HD):
    """(u1, u2, odd) of every element: the integer stream (oracle/philox_ref.py) and the kernel's float32 u = ((w >> 8) + 0.5) 2^-24"""
    from oracle.philox_ref import philox4x32_10
    e = np.arange(HD, dtype=np.uint32)
    smp = ((np.arange(B, dtype=np.uint64) + np.uint64(first)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    w = philox4x32_10((e >> np.uint32(2))[None, :], smp[:, None], np.uint32(step), np.uint32(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    comp = (e & np.uint32(3))[None, :]
    wa, wb = np.where(comp < 2, w[0], w[2]), np.where(comp < 2, w[1], w[3])
    u = lambda v: ((v >> np.uint32(8)).astype(F32) + F32(0.5)) * F32(2.0 ** -24)
    return u(wa), u(wb), np.broadcast_to((comp & 1) == 1, wa.shape)


def _philox_normal(inp, dt, ab):
    """Box-Muller of the two uniforms: z [B][HD]; ab: the radius times (|cos or sin| + the angle), the angle's own rounding
    reaching z through the other function"""
    B, HD = inp["B"], inp["H0"] * inp["D"]
    u1, u2, odd = _philox_uniforms(inp["seed"], inp["first"], B, inp["step"], HD)
    r = np.sqrt(dt(-2) * np.log(u1.astype(dt))).astype(dt)
    ang = (dt(TWO_PI_F32) * u2.astype(dt)).astype(dt)
    trig = np.where(odd, np.sin(ang), np.cos(ang)).astype(dt)
    return r * (np.abs(trig) + ang) + TINY if ab else (r * trig).astype(dt)


def _out_step(inp, dt, ab, seq, mutant):
    """eps = outc(feat) at the unpadded positions (mode 0: stored, nothing else); modes 1, 2: x <- scheduler step(x, eps), rows
    below inp_h overwritten by the in-painting rows, the new x also into history[step + 1]; flag = 1 when a stored value is not
    finite.  Non-finite stored values are reported in `nonfinite` (1 +inf, 2 -inf, 3 NaN) and zeroed in the other outputs."""
    B, H0, D, Hp, Wp, lh, lw, kind, mode, i = (inp[k] for k in ("B", "H0", "D", "Hp", "Wp", "lh", "lw", "kind", "mode", "step"))
    HD = H0 * D

    def classes(v):
        c = np.where(np.isnan(v), 3, np.where(v == np.inf, 1, np.where(v == -np.inf, 2, 0))).astype(dt)
        return c, np.where(c > 0, 0, v).astype(dt)

    eps = s_eps = None
    if mode != 2:
        f = inp["feat"].astype(dt).reshape(B, Hp, Wp, 64)[:, lh:lh + H0, lw:lw + D]
        w = inp["w"].astype(dt)
        bias = dt(0 if mutant == "bias_dropped" else inp["bias"])
        with np.errstate(invalid="ignore"):
            eps = (ssum(f * w, 3, seq) + bias).astype(dt)
            s_eps = ssum(np.abs(f) * np.abs(w), 3, False) + abs(bias)
    if mode == 0:
        cls, val = classes(eps)
        if ab:
            return {"eps": np.where(cls > 0, 0, s_eps), "nonfinite": np.zeros_like(cls), "flag": np.zeros(1, dt)}
        return {"eps": val, "nonfinite": cls, "flag": np.array([float(cls.any())], dt)}
    if mode == 2:
        eps = inp["eps"]
    elif inp.get("eps_dev") is not None and mutant != "bias_dropped":
        eps = inp["eps_dev"]                                   # the eps the eps-only mode of this launch produced
    else:                                                      # no device: the float64 eps rounded once, whatever dt is
        with np.errstate(invalid="ignore"):
            eps = (inp["feat"].astype(F64).reshape(B, Hp, Wp, 64)[:, lh:lh + H0, lw:lw + D] * inp["w"].astype(F64)).sum(3) + float(bias)
    eps = np.asarray(eps, F64).astype(F32).reshape(B, H0, D)
    c = inp["coef"][i]
    x = inp["x"].astype(F32).copy()
    rows = None
    if inp["inp_h"]:
        rows = inp["inpaint"].astype(F32)
        rows = rows if inp["inpaint_per_sample"] else np.broadcast_to(rows, (B,) + rows.shape[-2:])
    if mutant == "inpaint_before_update" and rows is not None:
        x[:, :inp["inp_h"]] = rows
    with np.errstate(invalid="ignore", over="ignore"):
        if mutant == "ddim_uses_x" and kind == 1:
            prev = c[2] * ((x - c[0] * eps) / c[1]) + c[4] * x
        else:
            prev = step_f32(kind, c, x, eps)                   # without the noise term
    s_prev = np.zeros((B, H0, D), F64)
    prev = prev.astype(dt)
    if kind == 0 and c[5] != 0:
        if inp["noise"] is not None:
            nz = inp["noise"].astype(F32)
            z = nz.reshape(-1, H0, D)[i + np.arange(B)] if mutant == "noise_sample_stride" else nz[i]
            prev = (prev.astype(F32) + c[5] * z).astype(dt)
        else:
            z = _philox_normal(inp, dt, ab).reshape(B, H0, D)
            if ab:
                s_prev = np.abs(prev) + abs(float(c[5])) * z
            else:
                prev = (prev + dt(c[5]) * z).astype(dt)
    if rows is not None and mutant != "inpaint_before_update":
        prev = prev.copy()
        prev[:, :inp["inp_h"]] = rows
        s_prev[:, :inp["inp_h"]] = 0
    cls, val = classes(prev)
    out = {"x": np.where(cls > 0, 0, s_prev) if ab else val, "nonfinite": np.zeros_like(cls) if ab else cls,
           "flag": np.zeros(1, dt) if ab else np.array([float(cls.any())], dt)}
    if inp["history"] is not None:
        h = np.zeros(inp["history"].shape, dt) if ab else inp["history"].astype(dt).copy()
        h[i if mutant == "history_slot_i" else i + 1] = out["x"]
        out["history"] = h
    return out


_IMPL = {"conv_in": _conv_in, "pool": _pool, "upcat": _upcat, "film_apply": _film_apply, "film_coef": _film_coef,
         "layernorm": _layernorm, "mish_pad": _padded(_mish), "silu_pad": _padded(_silu), "silu": _silu_flat,
         "dc_finish": _dc_finish, "simple_tail": _simple_tail, "splitk_combine": _splitk_combine, "out_step": _out_step}

_GN_MUTANTS = ("no_var_clamp", "slot_short_by_one", "cross_sample_slots", "cnorm_as_C")
MUTANTS = {
    "conv_in": ("part_dropped", "pad_offset_ignored", "no_zero_pad"),
    "pool": ("affine_after_max", "drop_odd_column") + _GN_MUTANTS,
    "upcat": ("align_corners_false", "concat_swapped", "no_edge_clamp", "skip_stats_from_up") + _GN_MUTANTS,
    "film_apply": ("temb_after_scale", "t_of_sample0", "row_stats_pre_film") + _GN_MUTANTS,
    "film_coef": ("mean_not_folded", "temb_after_scale", "t_of_sample0") + _GN_MUTANTS,
    "layernorm": ("no_eps", "drop_last_lane", "one_pass_variance"),
    "mish_pad": ("saturate_early", "kp_as_stride"),
    "silu_pad": ("saturate_early", "kp_as_stride"),
    "silu": ("saturate_early", "drop_last_block"),
    "dc_finish": ("res_after_gelu", "gelu_tanh") + _GN_MUTANTS,
    "simple_tail": ("gelu_after_temb", "pad_kept", "t_of_sample0") + _GN_MUTANTS,
    "splitk_combine": ("drop_last_slab", "drop_remainder_slab", "stats_first_pass_only"),
    "out_step": ("inpaint_before_update", "history_slot_i", "noise_sample_stride", "ddim_uses_x", "bias_dropped"),
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
        assert np.asarray(v).dtype == F32, (op, k, np.asarray(v).dtype)
    return {k: np.asarray(v, F64) for k, v in out.items()}


def tau(op, inp, r64=None, s64=None):
    return T.tau(op, inp, r64, s64, refs=(ref64, scale64, ref32, FLOOR_U))


# ---- data ------------------------------------------------------------------------------------------------------------------
GN_KINDS = (None, "serial", "mid", "wide", "straddle", "straddle_serial")
FLAVOURS = ("unit", "off10", "off300", "const")
GAINS = ("pos", "mixed", "neg", "zero")
LADDER = np.concatenate([EXTREMES, np.array([s * v for v in (5.99, 6.0, 6.01) for s in (1.0, -1.0)], F32)])


def _tensor(rng, fl, *shape):
    if fl == "off10":
        return (10 + 0.1 * rng.standard_normal(shape)).astype(F32)
    if fl == "off300":
        return (-300 + rng.standard_normal(shape)).astype(F32)
    if fl == "const":
        return np.full(shape, 10.0, F32)
    if fl == "ties":
        return np.round(np.clip(rng.standard_normal(shape), -1, 1)).astype(F32)
    if fl == "ladder":
        v = (8 * rng.standard_normal(shape)).astype(F32)
        flat = v.reshape(-1)
        flat[:min(len(LADDER), flat.size)] = LADDER[:flat.size]
        return v
    return _randn(rng, *shape)


def _gain(rng, kind, C):
    if kind == "neg":
        return (-1 - 0.3 * np.abs(rng.standard_normal(C))).astype(F32)
    if kind == "zero":
        return np.zeros(C, F32)
    if kind == "mixed":
        return _edge_gain(rng, C)
    return (1 + 0.3 * rng.standard_normal(C)).astype(F32)


def _make_gn(rng, x, kind, fl, gain, cnorm=None, n_affine=None):
    """The pending GroupNorm of x [B][HW][C] (None: x is final).  cnorm < C: padded storage -- lanes [cnorm, C) of x are set to
    exact zeros, as are gamma and beta there.  fl 'const': the partials as a producer that accumulates in float32 leaves them,
    sum x^2 low by 2^-22 of itself, so that E[x^2] - mean^2 is negative."""
    if kind is None:
        return None
    B, HW, C = x.shape
    cnorm = cnorm or C
    x[:, :, cnorm:] = 0
    m_tile, n_tiles = gn_geometry(kind, HW)
    reads = gn_reads(B, HW, m_tile, n_tiles)
    want = {"serial": lambda n: n <= 8, "mid": lambda n: 9 <= n <= 64, "wide": lambda n: n >= 65,
            "straddle": lambda n: HW % m_tile != 0 and B >= 3 and 9 <= n <= 64,
            "straddle_serial": lambda n: HW % m_tile != 0 and B >= 3 and n <= 8}[kind]
    assert all(want(n) for n in reads), (kind, HW, reads)
    st = make_partials(x, m_tile, n_tiles)
    if fl == "const":
        st[:, :, 1] *= 1 - 2.0 ** -22
    n_affine = n_affine or C
    ga, be = _gain(rng, gain, n_affine), (0.3 * rng.standard_normal(n_affine)).astype(F32)
    ga[cnorm:] = 0
    be[cnorm:] = 0
    return dict(stats=st, slots=st.shape[1], m_tile=m_tile, n_tiles=n_tiles, cnorm=cnorm, HW=HW, C=C, gamma=ga, beta=be)


def _timesteps(t_count, T_):
    """distinct timesteps with both ends of the table"""
    return np.array({1: [T_ - 1], 2: [0, T_ - 1], 3: [T_ - 1, 0, 3]}[t_count], np.int32)


def _gn_cycle(i, B, HW):
    """the i-th (kind, flavour, gain) of the cycle that fits the shape"""
    kinds = [k for k in GN_KINDS if not (str(k).startswith("straddle") and (B < 3 or HW < 3)) and not (k == "wide" and HW < 2)]
    return kinds[i % len(kinds)], FLAVOURS[(i // 2) % len(FLAVOURS)], GAINS[(i // 3) % len(GAINS)]


def cases(op):
    """[(case id, parameters)]: the shapes and flavours of one op."""
    C_ = []
    add = lambda cid, **kw: C_.append((cid, kw))
    if op == "conv_in":
        i = 0
        for H0, D in ((8, 1), (16, 3), (31, 5), (64, 6)):
            for B in (1, 3):
                for Bg in (0, 1024):
                    adv = (-2, -1, 2)[i % 3]
                    n_steps, step0 = (0, 0) if adv == -2 else (5, (4, 1)[i % 2])   # step0 + 1 == n_steps: the clamped read
                    add(f"h{H0}d{D}_b{B}_g{Bg}_adv{adv}_s{step0}", H0=H0, D=D, B=B, B_geom=Bg, adv=adv, n_steps=n_steps,
                        step0=step0, flavour="unit", parts=1 if Bg else 4)
                    i += 1
        add("h16d3_b2_offset", H0=16, D=3, B=2, B_geom=0, adv=5, n_steps=5, step0=0, flavour="off10", parts=4)
        add("h8d8_b2_full_width", H0=8, D=8, B=2, B_geom=0, adv=-2, n_steps=0, step0=0, flavour="unit", parts=4)   # data up to the border
        add("h31d5_b2_zero", H0=31, D=5, B=2, B_geom=0, adv=-1, n_steps=3, step0=2, flavour="zero", parts=4)
    elif op == "pool":
        i = 0
        for C in (64, 128, 192, 256, 512):
            for H, W in ((2, 2), (8, 2), (16, 8), (6, 4)):
                for B in (1, 3):
                    kind, fl, gain = _gn_cycle(i, B, H * W)
                    add(f"c{C}_{H}x{W}_b{B}_{kind}_{fl}_{gain}", C=C, H=H, W=W, B=B, gn=kind, flavour=fl, gain=gain)
                    i += 1
        add("c64_16x8_b3_none_ties", C=64, H=16, W=8, B=3, gn=None, flavour="ties", gain="pos")
        add("c192_6x4_b3_straddle_neg", C=192, H=6, W=4, B=3, gn="straddle", flavour="unit", gain="neg")
        add("c64_8x2_b2_mid_const", C=64, H=8, W=2, B=2, gn="mid", flavour="const", gain="mixed")
        add("c128_8x2_b2_wide_cnorm96", C=128, H=8, W=2, B=2, gn="wide", flavour="unit", gain="pos", cnorm=96)
        add("c64_6x4_b3_serial_ties_neg", C=64, H=6, W=4, B=3, gn="serial", flavour="ties", gain="neg")
    elif op == "upcat":
        i = 0
        # (Cu, Cs): equal widths (the split thread map), no skip, and simple_Unet's padded concatenations up3, up1, up2
        for Cu, Cs in ((64, 64), (256, 256), (192, 192), (128, 64), (64, 0), (320, 192), (192, 64)):
            for Hin, Win in ((1, 1), (1, 4), (4, 1), (2, 2), (4, 4), (8, 4), (3, 5)):
                B = (1, 3)[i % 2]
                kind, fl, gain = _gn_cycle(i, B, Hin * Win)
                ks = _gn_cycle(i + 2, B, 4 * Hin * Win)[0] if Cs else None
                add(f"u{Cu}s{Cs}_{Hin}x{Win}_b{B}_{kind}_{ks}_{fl}_{gain}", Cu=Cu, Cs=Cs, Hin=Hin, Win=Win, B=B, gn=kind, gn_skip=ks,
                    flavour=fl, gain=gain)
                i += 1
        add("u64s64_4x4_b3_straddle_wide_const", Cu=64, Cs=64, Hin=4, Win=4, B=3, gn="straddle", gn_skip="wide", flavour="const", gain="mixed")
        add("u128s64_3x5_b2_mid_mid_cnorm", Cu=128, Cs=64, Hin=3, Win=5, B=2, gn="mid", gn_skip="mid", flavour="unit", gain="pos", cnorm=100,
            cnorm_skip=40)
    elif op in ("film_apply", "film_coef"):
        i = 0
        Cs = (64, 128, 256, 512, 32) if op == "film_apply" else (64, 128, 192, 256, 512)
        for C in Cs:
            for HW in (1, 5, 17, 64):
                B = (2, 3)[i % 2]
                kind, fl, gain = _gn_cycle(i, B, HW)
                tc = (1, B)[i % 2]
                add(f"c{C}_hw{HW}_b{B}_{kind}_{fl}_{gain}_t{tc}", C=C, HW=HW, B=B, gn=kind, flavour=fl, gain=gain, t_count=tc, temb=True,
                    film=True, row_stats=op == "film_apply" and C in (64, 128, 256))
                i += 1
        base = dict(C=64, HW=17, B=3, gn="mid", flavour="unit", gain="mixed", t_count=3, temb=True, film=True, row_stats=op == "film_apply")
        add("no_temb", **{**base, "temb": False, "t_count": 1})
        add("no_film", **{**base, "film": False})
        add("no_gn", **{**base, "gn": None})
        add("gn_only", **{**base, "temb": False, "film": False, "t_count": 1, "row_stats": False})
        add("all_absent", **{**base, "temb": False, "film": False, "gn": None, "t_count": 1, "row_stats": False})
        add("const_wide", **{**base, "gn": "wide", "flavour": "const"})
        add("cnorm", **{**base, "C": 128, "cnorm": 80, "gn": "straddle"})
    elif op == "layernorm":
        for C in (64, 128, 256, 512):
            for rows in (1, 4, 5, 67):
                add(f"c{C}_r{rows}", C=C, rows=rows, flavour="unit")
            add(f"c{C}_r5_offsets", C=C, rows=5, flavour="offsets")
            add(f"c{C}_r4_off300", C=C, rows=4, flavour="off300")
    elif op in ("mish_pad", "silu_pad"):
        for B, cd, Kp in ((1, 30, 32), (3, 30, 30), (3, 37, 64), (2, 128, 128), (5, 70, 96)):
            add(f"b{B}_d{cd}_k{Kp}", B=B, cond_dim=cd, Kp=Kp, flavour="ladder")
        add("b3_d37_k64_unit", B=3, cond_dim=37, Kp=64, flavour="unit")
    elif op == "silu":
        for n in (1, 255, 256, 257, 1000):
            add(f"n{n}", n=n, flavour="ladder")
        add("n1000_unit", n=1000, flavour="unit")
    elif op == "dc_finish":
        i = 0
        for C in (64, 192, 512):
            for HW in (1, 5, 17, 64):
                B = (2, 3)[i % 2]
                kind, fl, gain = _gn_cycle(i, B, HW)
                add(f"c{C}_hw{HW}_b{B}_{kind}_{fl}_{gain}_r{i % 2}", C=C, HW=HW, B=B, gn=kind, flavour=fl, gain=gain, res=bool(i % 2))
                i += 1
        base = dict(C=64, HW=17, B=3, gn=None, flavour="ladder", gain="pos", res=False)
        add("ladder", **base)
        add("ladder_res", **{**base, "res": True})
        add("c192_ladder", **{**base, "C": 192})
        add("const_wide", **{**base, "gn": "wide", "flavour": "const", "gain": "mixed", "res": True})
        add("cnorm", **{**base, "C": 128, "cnorm": 80, "gn": "straddle", "flavour": "unit", "res": True})
    elif op == "simple_tail":
        i = 0
        # (Co, Cr, src_C, temb_ld): Cr + 32 == Co and < Co, src_C > Cr, temb_ld > Cr
        for Co, Cr, sC, tld in ((64, 4, 64, 4), (64, 32, 32, 32), (128, 96, 128, 96), (128, 32, 64, 40), (192, 96, 128, 128)):
            for HW in (1, 5, 17, 64):
                B = (2, 3)[i % 2]
                kind, fl, gain = _gn_cycle(i, B, HW)
                tc = (1, B)[i % 2]
                add(f"o{Co}r{Cr}s{sC}l{tld}_hw{HW}_b{B}_{kind}_{fl}_{gain}_t{tc}", Co=Co, Cr=Cr, src_C=sC, temb_ld=tld, cemb_ld=(32, 48)[i % 2],
                    HW=HW, B=B, gn=kind, flavour=fl, gain=gain, t_count=tc)
                i += 1
        base = dict(Co=64, Cr=32, src_C=32, temb_ld=32, cemb_ld=32, HW=17, B=3, gn=None, flavour="ladder", gain="pos", t_count=3)
        add("ladder", **base)
        add("const_wide", **{**base, "gn": "wide", "flavour": "const", "gain": "mixed"})
        add("straddle_unit", **{**base, "gn": "straddle", "flavour": "unit", "gain": "mixed", "Co": 128, "src_C": 64})
    elif op == "splitk_combine":
        i = 0
        for ks in (2, 3, 4, 5, 6, 9):
            for HW, N in ((4, 64), (16, 256), (64, 512), (9, 512), (25, 512), (64, 64)):
                if (i + ks) % 2 == 0 or (HW, N) == (25, 512) and ks in (2, 9):
                    add(f"k{ks}_hw{HW}_n{N}_b{(1, 3)[i % 2]}", ksplit=ks, HW=HW, N=N, B=(1, 3)[i % 2], flavour=("unit", "cancel")[i % 3 == 0])
                i += 1
    elif op == "out_step":
        # n_steps 5 of T 20: timesteps 16, 12, 8, 4, 0 -- the last step has k_noise == 0
        base = dict(kind=0, mode=2, step=2, noise="buffer", inp_h=0, per_sample=0, history=True, indirect=0, flavour="unit")
        shapes = ((8, 1, 1), (16, 3, 3), (31, 5, 2))
        i = 0
        for H0, D, B in shapes:
            for mode in (0, 1, 2):
                for kind in (0, 1):
                    kw = dict(base, H0=H0, D=D, B=B, mode=mode, kind=kind, step=(0, 2, 4)[i % 3], indirect=i % 2, history=i % 3 != 1,
                              inp_h=(0, 1, H0)[i % 3], per_sample=(i // 2) % 2, noise=("buffer", "philox")[i % 2] if kind == 0 else "none")
                    add(f"h{H0}d{D}b{B}_m{mode}_k{kind}_s{kw['step']}_{kw['noise']}_i{kw['inp_h']}p{kw['per_sample']}_h{int(kw['history'])}_x{kw['indirect']}", **kw)
                    i += 1
        b2 = dict(base, H0=16, D=3, B=3)
        add("philox_mid_direct", **{**b2, "noise": "philox", "step": 1})
        add("philox_first_indirect_inp4", **{**b2, "noise": "philox", "step": 0, "indirect": 1, "inp_h": 4, "per_sample": 1})
        add("ddpm_last_step_no_noise", **{**b2, "noise": "none", "step": 4})
        add("ddpm_last_step_buffer_unused", **{**b2, "noise": "buffer", "step": 4, "mode": 1})
        add("ddpm_buffer_inp1_shared_indirect", **{**b2, "inp_h": 1, "indirect": 1, "mode": 1})
        add("ddpm_buffer_inpH0_per_sample", **{**b2, "inp_h": 16, "per_sample": 1})
        add("ddim_mid_from_features", **{**b2, "kind": 1, "noise": "none", "mode": 1, "history": False})
        add("nonfinite_features_full_step", **{**b2, "mode": 1, "flavour": "nonfinite", "inp_h": 1})
        add("nonfinite_features_eps_only", **{**b2, "mode": 0, "flavour": "nonfinite"})
    else:
        raise KeyError(op)
    return C_


def make_inputs(op, case):
    """The float32 (and integer) inputs of one case, with its parameters."""
    cid, kw = case
    rng = np.random.default_rng(_seed(op, cid))
    fl = kw["flavour"]
    inp = dict(kw)
    if op == "conv_in":
        B, H0, D = kw["B"], kw["H0"], kw["D"]
        Hp, Wp = -(-H0 // 8) * 8, -(-D // 8) * 8          # the engine's padding: up to a multiple of 8, the data centred
        inp.update(Hp=Hp, Wp=Wp, lh=(Hp - H0) // 2, lw=(Wp - D) // 2)
        inp["x"] = np.zeros((B, H0, D), F32) if fl == "zero" else _tensor(rng, fl, B, H0, D)
        inp["w"] = _randn(rng, 9, 64)
        inp["timesteps"] = np.arange(kw["n_steps"] - 1, -1, -1, dtype=np.int32) * 7 + 3
        assert conv_in_parts(Hp * Wp, kw["B_geom"] or B) == kw["parts"]
    elif op == "pool":
        B, H, W, C = kw["B"], kw["H"], kw["W"], kw["C"]
        x = _tensor(rng, fl, B, H * W, C)
        inp["gn"] = _make_gn(rng, x, kw["gn"], fl, kw["gain"], kw.get("cnorm"))
        inp["x"] = x
    elif op == "upcat":
        B, Hin, Win, Cu, Cs = kw["B"], kw["Hin"], kw["Win"], kw["Cu"], kw["Cs"]
        up = _tensor(rng, fl, B, Hin * Win, Cu)
        inp["gn"] = _make_gn(rng, up, kw["gn"], fl, kw["gain"], kw.get("cnorm"))
        inp["up"] = up
        inp["skip"] = inp["gn_skip"] = None
        if Cs:
            skip = _tensor(rng, "unit" if fl == "const" else fl, B, 4 * Hin * Win, Cs) + F32(1.5)
            inp["gn_skip"] = _make_gn(rng, skip, kw["gn_skip"], "unit", kw["gain"], kw.get("cnorm_skip"))
            inp["skip"] = skip
    elif op in ("film_apply", "film_coef", "dc_finish"):
        B, HW, C = kw["B"], kw["HW"], kw["C"]
        x = _tensor(rng, fl, B, HW, C)
        inp["gn"] = _make_gn(rng, x, kw["gn"], fl, kw["gain"], kw.get("cnorm"))
        inp["x"] = x
        if op == "dc_finish":
            inp["res"] = _randn(rng, B, HW, C) if kw["res"] else None
        else:
            T_ = 7
            inp["T"] = T_
            inp["temb"] = _randn(rng, T_, C) if kw["temb"] else None
            inp["film"] = (_randn(rng, B, 2 * C) * F32(1.0)) if kw["film"] else None
            inp["t"] = _timesteps(kw["t_count"], T_) if kw["temb"] else None
    elif op == "layernorm":
        rows, C = kw["rows"], kw["C"]
        if fl == "offsets":
            x = T._edges(rng, 1, rows, C)[0]
            x[-1] = 0
            x[1], x[2], x[3] = 7.25, 100.3, 57.7           # constant rows: variance 0, only eps is left
        else:
            x = _tensor(rng, fl, rows, C)
        inp["x"] = x
        inp["g"] = _edge_gain(rng, C) if fl != "unit" else _gain(rng, "pos", C)
        inp["b"] = (0.3 * rng.standard_normal(C)).astype(F32)
    elif op in ("mish_pad", "silu_pad"):
        inp["cond"] = _tensor(rng, fl, kw["B"], kw["cond_dim"])
    elif op == "silu":
        inp["x"] = _tensor(rng, fl, kw["n"])
    elif op == "simple_tail":
        B, HW, Cr, sC = kw["B"], kw["HW"], kw["Cr"], kw["src_C"]
        x = _tensor(rng, fl, B, HW, sC)
        x[:, :, Cr:] = 0
        inp["gn"] = _make_gn(rng, x, kw["gn"], fl, kw["gain"], cnorm=Cr if kw["gn"] else None, n_affine=Cr)
        inp["x"] = x
        T_ = 7
        inp["T"] = T_
        inp["temb"] = _randn(rng, T_, kw["temb_ld"])
        inp["cemb"] = _randn(rng, B, kw["cemb_ld"])
        inp["t"] = _timesteps(kw["t_count"], T_)
    elif op == "splitk_combine":
        B, HW, N, ks = kw["B"], kw["HW"], kw["N"], kw["ksplit"]
        p = _randn(rng, ks, B * HW, N)
        if fl == "cancel":                                 # large slabs of opposite sign: the sum is what is left of them
            big = _randn(rng, B * HW, N, scale=1e4)
            p[0] += big
            p[-1] -= big
        inp["partial"] = p
    elif op == "out_step":
        B, H0, D, kind = kw["B"], kw["H0"], kw["D"], kw["kind"]
        Hp, Wp = -(-H0 // 8) * 8, -(-D // 8) * 8
        n, T_ = 5, 20
        inp.update(Hp=Hp, Wp=Wp, lh=(Hp - H0) // 2, lw=(Wp - D) // 2, n_steps=n, inpaint_per_sample=kw["per_sample"],
                   bias=float(F32(0.37)), seed=(0x9E3779B9 << 32) | 0x01234567, first=5)
        inp["coef"], inp["timesteps"] = coef_table(kind, T_, n)
        inp["feat"], inp["w"] = _randn(rng, B, Hp * Wp, 64), _randn(rng, 64, scale=0.2)
        inp["x"], inp["eps"] = _randn(rng, B, H0, D), _randn(rng, B, H0, D)
        inp["noise"] = _randn(rng, n, B, H0, D) if kw["noise"] == "buffer" else None
        inp["inpaint"] = _randn(rng, *((B,) if kw["per_sample"] else ()), kw["inp_h"], D) if kw["inp_h"] else None
        inp["history"] = _randn(rng, n + 1, B, H0, D) if kw["history"] else None
        if fl == "nonfinite":                                  # one infinite and one NaN feature: ordinary data
            f = inp["feat"].reshape(B, Hp, Wp, 64)
            f[0, inp["lh"] + 2, inp["lw"] + 1, 5] = np.inf
            f[B - 1, inp["lh"] + 7, inp["lw"], 41] = np.nan
        if kw["mode"] == 1:                                    # on the CPU: the float64 eps rounded; on the device: its own mode-0 eps
            inp["eps_dev"] = None
    else:
        raise KeyError(op)
    return inp


# ---- the launch of one case through spdm_op_stream (include/spdm.h) -----------------------------------------------------------
def launch_plan(op, inp):
    """The hook's arguments of one case: dims; bufs -- ("in" | "inout", float32 array), ("out", elements) or None; idx (int32 array
    or None); gn -- [the pending GroupNorm of source k or None]; stats_out (doubles or None); words (bool); outs -- {name: (source,
    shape, row stride or None)} with source a buffer index, "stats" or "words" (a stride: rows of that many elements of which the
    first prod(shape[1:]) are written, the rest left as they were)."""
    g = lambda *names: [int(inp[n]) for n in names]
    I, O = (lambda a: ("in", np.ascontiguousarray(a, F32))), (lambda n: ("out", int(n)))
    P = dict(idx=None, gn=[None, None], stats_out=None, words=False)
    if op == "conv_in":
        P["dims"] = g("B", "H0", "D", "Hp", "Wp", "lh", "lw", "B_geom", "adv", "n_steps", "step0")
        B, HW = inp["B"], inp["Hp"] * inp["Wp"]
        parts = inp["parts"]
        slots = stats_slots(HW, HW // parts, 1)
        P["bufs"] = [I(inp["x"]), I(inp["w"]), O(B * HW * 64)]
        P["stats_out"] = B * slots * 2
        P["outs"] = {"dst": (2, (B, HW, 64), None), "stats": ("stats", (B, parts, 2), slots * 2)}
        if inp["adv"] >= -1:
            P["idx"], P["words"] = inp["timesteps"], True
            P["outs"]["words"] = ("words", (2,), None)
    elif op == "pool":
        B, H, W, C = P["dims"] = g("B", "H", "W", "C")
        P["bufs"], P["gn"][0] = [I(inp["x"]), O(B * H * W * C // 4)], inp["gn"]
        P["outs"] = {"dst": (1, (B, H * W // 4, C), None)}
    elif op == "upcat":
        B, Hin, Win, Cu, Cs = P["dims"] = g("B", "Hin", "Win", "Cu", "Cs")
        n = B * 4 * Hin * Win * (Cu + Cs)
        P["bufs"] = [I(inp["up"]), I(inp["skip"]) if Cs else None, O(n)]
        P["gn"] = [inp["gn"], inp["gn_skip"]]
        P["outs"] = {"dst": (2, (B, 4 * Hin * Win, Cu + Cs), None)}
    elif op in ("film_apply", "film_coef"):
        B, HW, C = g("B", "HW", "C")
        P["dims"] = [B, HW, C, int(inp["t_count"]), int(inp["T"]) if inp["temb"] is not None else 1]
        opt = lambda a: None if a is None else I(a)
        P["gn"][0], P["idx"] = inp["gn"], inp["t"]
        if op == "film_apply":
            P["bufs"] = [I(inp["x"]), opt(inp["temb"]), opt(inp["film"]), O(B * HW * C)]
            P["outs"] = {"dst": (3, (B, HW, C), None)}
            if inp["row_stats"]:
                P["stats_out"] = B * HW * 2
                P["outs"]["row_stats"] = ("stats", (B, HW, 2), None)
        else:
            P["bufs"] = [opt(inp["temb"]), opt(inp["film"]), O(B * 2 * C)]
            P["outs"] = {"ab": (2, (B, 2 * C), None)}
    elif op == "layernorm":
        rows, C = P["dims"] = g("rows", "C")
        P["bufs"], P["outs"] = [I(inp["x"]), I(inp["g"]), I(inp["b"]), O(rows * C)], {"y": (3, (rows, C), None)}
    elif op in ("mish_pad", "silu_pad"):
        B, cd, Kp = P["dims"] = g("B", "cond_dim", "Kp")
        P["bufs"], P["outs"] = [I(inp["cond"]), O(B * Kp)], {"dst": (1, (B, Kp), None)}
    elif op == "silu":
        n, = P["dims"] = g("n")
        P["bufs"], P["outs"] = [I(inp["x"]), O(n)], {"y": (1, (n,), None)}
    elif op == "dc_finish":
        B, HW, C = P["dims"] = g("B", "HW", "C")
        P["bufs"] = [I(inp["x"]), I(inp["res"]) if inp["res"] is not None else None, O(B * HW * C)]
        P["gn"][0], P["outs"] = inp["gn"], {"dst": (2, (B, HW, C), None)}
    elif op == "simple_tail":
        B, HW, Co, Cr, sC, tld, cld, tc, T_ = P["dims"] = g("B", "HW", "Co", "Cr", "src_C", "temb_ld", "cemb_ld", "t_count", "T")
        S = lambda a, ld, width: ("in", np.ascontiguousarray(a, F32).reshape(-1, ld).ravel()[:a.size - ld + width])
        P["bufs"] = [I(inp["x"]), S(inp["temb"], tld, Cr), S(inp["cemb"], cld, 32), O(B * HW * Co)]
        P["gn"][0], P["idx"], P["outs"] = inp["gn"], inp["t"], {"dst": (3, (B, HW, Co), None)}
    elif op == "splitk_combine":
        B, HW, N, ks = P["dims"] = g("B", "HW", "N", "ksplit")
        rows = combine_rows(HW, N)
        slots = stats_slots(HW, rows, 1)
        P["bufs"], P["stats_out"] = [I(inp["partial"]), O(B * HW * N)], B * slots * 2
        P["outs"] = {"dst": (1, (B * HW, N), None), "stats": ("stats", (B, HW // rows, 2), slots * 2)}
    elif op == "out_step":
        B, H0, D, Hp, Wp = g("B", "H0", "D", "Hp", "Wp")
        mode, n = int(inp["mode"]), int(inp["n_steps"])
        P["dims"] = g("B", "H0", "D", "Hp", "Wp", "lh", "lw", "kind", "mode", "step", "n_steps", "inp_h", "inpaint_per_sample", "indirect")
        opt = lambda a, kind="in": None if a is None else (kind, np.ascontiguousarray(a, F32))
        E = B * H0 * D
        if mode == 0:
            P["bufs"] = [I(inp["feat"]), I(inp["w"]), O(E)]
            P["outs"] = {"eps": (2, (B, H0, D), None)}
        else:
            feat = mode == 1
            P["bufs"] = [I(inp["feat"]) if feat else None, I(inp["w"]) if feat else None, None if feat else I(inp["eps"]),
                         ("inout", inp["x"]), I(inp["coef"]), opt(inp["noise"]), opt(inp["inpaint"]), opt(inp["history"], "inout")]
            P["outs"] = {"x": (3, (B, H0, D), None)}
            if inp["history"] is not None:
                P["outs"]["history"] = (7, (n + 1, B, H0, D), None)
        P["outs"]["flag"] = ("flag", (1,), None)
        P.update(words=True, bias=inp["bias"], seed=inp["seed"], first=inp["first"])
    else:
        raise KeyError(op)
    if P["idx"] is not None:
        P["idx"] = np.ascontiguousarray(P["idx"], np.int32)
    return P


def finish_got(op, got):
    """The launch's outputs as the references report them: out_step's non-finite stored values as classes, zeroed elsewhere."""
    if op != "out_step":
        return got
    got = dict(got)
    main = got["x" if "x" in got else "eps"]
    cls = np.where(np.isnan(main), 3, np.where(main == np.inf, 1, np.where(main == -np.inf, 2, 0))).astype(F64)
    got["nonfinite"] = cls
    for k in ("x", "eps", "history"):
        if k in got:
            got[k] = np.where(np.isfinite(got[k]), got[k], 0)
    return got


def expected_info(op, inp):
    """info[] the hook reports: {row parts, slots} of conv_in, {rows per workgroup, slots} of the split-K combine; None otherwise."""
    if op == "conv_in":
        HW = inp["Hp"] * inp["Wp"]
        parts = conv_in_parts(HW, inp["B_geom"] or inp["B"])
        return parts, stats_slots(HW, HW // parts, 1)
    if op == "splitk_combine":
        rows = combine_rows(inp["HW"], inp["N"])
        return rows, stats_slots(inp["HW"], rows, 1)
    return None
