"""Plain CPU references of ONE forward SelfAttention launch (spdm_op_sa, include/spdm.h), for tests only.  tests/sa_ref.py stays
the single float64 definition of a block: ref64 of a whole-block launch IS sa_block_ref on the (ab-affine or FiLM'd) input, and
the restatement below -- one forward written once over a small arithmetic interface -- is held to it by
tests/test_sa_ops_reference.py before it serves as ref32, ref_split, the mutants and the partial ops' slices.

  ref64(op, inp)       the launch in float64.  FUSED64 and the chains: sa_block_ref; with a crop the tokens (lh + i) Wp + lw + j,
                       with outc eps = out . w + b.  QKV / CORE / HEAD / TAIL: the corresponding slice of the block's intermediates.
  bound(op, inp)       whole block: sa_ref.sa_bound, TAU and TAU_S unchanged (with outc: carried through |outc_w|, plus the dot
                       product's own term by tests/stream_ops_ref.py's out_step rule).  Partial op: TAU_op S_op, S_op the launch's
                       expression with every term in absolute value -- LayerNorm's (v - mu) counts |v| + |mu| -- and the softmax
                       contributing sa_ref's S V term; TAU_op = train_ops_ref.tau over TWO restatements, references alone:
  ref32(op, inp)       (a) the same formulas in float32 with every sum taken sequentially;
  ref_split(op, inp)   (b) a float64 model of the documented number format of each product (DESIGN.md 4.1, 4.3, 4.3b and the
                       headers of sa_fused.hip, sa_tail.hip, attention.hip): each operand a pre-scaled fp16 hi + lo (activations
                       x 16, weights x 128, probabilities x 1024; sa_ref._r16), the lo lo term dropped, 32 products at a time
                       added into a float32 accumulator; gemm_ref.floor_terms' floors where a lo half can be an fp16 subnormal.
  MUTANTS[op]          float64 models of the mistakes a kernel could make.

Admission of data: a case is kept only if a PLAIN float32 CPU evaluation of the same op lies within ADMIT = 0.5 of the bound on
every element (tests/test_sa_ops_reference.py asserts it for every case): the tests then fail on a kernel, not on conditioning.
Per-sample means of 10 .. 300 are admitted although the residual |x| in A makes the bound loose there.

cases(op) is the table the CPU and GPU tests share, make_inputs(op, case) the data, chain_inputs(route, C) the chains' first link.
"""
import json
import math
import os

import numpy as np
import torch

import sa_ref
import stream_ops_ref as S
import train_ops_ref as T
from gemm_ref import floor_terms
from sa_ref import HEADS, sa_block_ref, sa_bound
from train_ops_ref import F32, F64, U, _seed

OPS = ("fused64", "qkv", "head", "tail", "core")
KERNELS = ("fused", "fused_pair", "crop", "qkv", "head", "tail", "core_ds", "core_valu", "core_mfma")
ADMIT = 0.5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sa_ops_tau.json")
BLOCK_OF = {64: "sa6", 128: "sa1", 256: "sa2"}
EPS = 1e-5
A_SCALE, W_SCALE, P_SCALE = 16.0, 128.0, 1024.0
# Floors of TAU_op in units of u: only the roundings on one element's chain that NEITHER restatement carries (both carry every sum,
# the LayerNorm arithmetic, the stores and libm's exp / erf), i.e. where the kernels may use another instruction than numpy:
#   qkv   A x + B contracted into one FMA (1), rstd through v_rsq_f32, 1 ulp (2), the bias added in another place (1)
#   core  exp through v_exp_f32 with a compensated argument (2 + 1), 1 / den through v_rcp_f32 (2), the final scale (1)
#   head  both
#   tail  the FMA (1), v_rsq_f32 (2), the device erf, <= 2 ulp from erff (4), the residual added in another place (1)
FLOOR_U = {"qkv": 4, "core": 6, "head": 10, "tail": 8}
_W = {}


def block_weights(C, flavour):
    """{short name: float32 array} of a random block with C channels, its q / k rows sharpened (sa_ref.FLAVOURS)"""
    key = (C, flavour)
    if key not in _W:
        sd, name = sa_ref.flavour_weights(flavour), BLOCK_OF[C]
        _W[key] = {k[len(name) + 1:]: np.asarray(v, F32) for k, v in sd.items() if k.startswith(name + ".")}
    return _W[key]


def _sd(W):
    return {"b." + k: torch.from_numpy(v) for k, v in W.items()}


# ---- the arithmetic a forward is written over ------------------------------------------------------------------------------
class N64:
    """float64, numpy's own sums"""
    dt = F64

    def arr(self, v):
        return np.asarray(v, self.dt)

    def dot(self, x, w, kind="aw"):                    # x [..., K] . w [N, K] -> [..., N]
        return x @ w.T

    def mean(self, x):
        return x.mean(-1, keepdims=True)

    def exp(self, x):
        return np.exp(x)

    def keysum(self, p):
        return p.sum(-1, keepdims=True)

    def pv(self, p, v):                                # p [..., Lq, Lk], v [..., Lk, d]
        return p @ v

    def qk(self, q, k):
        return q @ np.swapaxes(k, -1, -2)

    def erf(self, x):
        return T._erf(x)


class N32(N64):
    """float32, every sum sequential"""
    dt = F32

    def _seq(self, a, b):                              # a [..., M, K] b [..., N, K] -> a b^T, one product and one add per k
        acc = np.zeros(np.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-2]), F32)
        for k in range(a.shape[-1]):
            acc = acc + a[..., :, k, None] * b[..., None, :, k]
        return acc

    def dot(self, x, w, kind="aw"):
        return self._seq(x, w)

    def mean(self, x):
        return (T.ssum(x, -1, True) * F32(1.0 / x.shape[-1]))[..., None]

    def keysum(self, p):
        return T.ssum(p, -1, True)[..., None]

    def pv(self, p, v):
        return self._seq(p, np.swapaxes(v, -1, -2))

    def qk(self, q, k):
        return self._seq(q, k)


def _r16(z, scale):
    return sa_ref._r16(torch.from_numpy(np.ascontiguousarray(z, F64)), scale).numpy()


def _split(z, scale):
    hi = _r16(z, scale)
    return hi, _r16(z - hi, scale)


class NSplit(N64):
    """float64 model of the split-fp16 products: a b ~ ah bh + ah bl + al bh, 32 products per step into a float32 accumulator;
    every stored intermediate is a float32"""
    dt = F64
    SC = {"a": A_SCALE, "w": W_SCALE, "p": P_SCALE}

    def _acc(self, a, b, sa, sb):
        ah, al = _split(a, sa)
        bh, bl = _split(b, sb)
        K = a.shape[-1]
        t = lambda z: np.swapaxes(z, -1, -2)
        acc = np.zeros(np.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-2]), F32)
        for k in range(0, K, 32):
            s = slice(k, min(k + 32, K))
            part = ah[..., s] @ t(bh[..., s]) + ah[..., s] @ t(bl[..., s]) + al[..., s] @ t(bh[..., s])
            acc = (acc.astype(F64) + part).astype(F32)
        return acc.astype(F64)

    def dot(self, x, w, kind="aw"):                    # a [..., M, K] b [..., N, K] -> a b^T
        return self._acc(x, w, self.SC[kind[0]], self.SC[kind[1]])

    def qk(self, q, k):
        return self._acc(q, k, A_SCALE, A_SCALE)

    def pv(self, p, v):
        return self._acc(p, np.swapaxes(v, -1, -2), P_SCALE, A_SCALE)

    def arr(self, v):
        return np.asarray(v, F64)


def _store(n, v):
    """a value the kernels hold as a float32 (the format model only: float64 stays exact, float32 is one already)"""
    return v.astype(F32).astype(F64) if isinstance(n, NSplit) else v


def _ln(n, v, g, b):
    mu = n.mean(v)
    d = v - mu
    var = n.mean(d * d)
    return d * (1 / np.sqrt(var + n.dt(EPS))) * g + b


def _attn(n, q, k, v, mutant=None, per=0):
    """softmax(q k^T / sqrt d) v per (sample, head); q, k, v [B, L, C] -> [B, L, C]"""
    B, L, C = q.shape
    d = C // HEADS
    hd = lambda z: z.reshape(B, L, HEADS, d).transpose(0, 2, 1, 3)
    q, k, v = hd(q) * n.dt(1 / math.sqrt(d)), hd(k), hd(v)
    if mutant in ("q_fp16", "k_fp16", "v_fp16"):
        q, k, v = (_r16(z, 16.0) if mutant[0] == nm else z for z, nm in ((q, "q"), (k, "k"), (v, "v")))
    lg = _store(n, n.qk(q, k))
    if mutant == "key_tail_unmasked" and L % 32:       # the padded keys of the last 32-key block: k = v = 0, logit 0
        pad = 32 - L % 32
        lg = np.concatenate([lg, np.zeros(lg.shape[:-1] + (pad,), lg.dtype)], -1)
        v = np.concatenate([v, np.zeros(v.shape[:-2] + (pad, d), v.dtype)], -2)
    if mutant == "skip_rescale":
        o = sa_ref._online(torch.from_numpy(lg * sa_ref.LOG2E), torch.from_numpy(v), 1.0).numpy()
    else:
        pu = _store(n, n.exp(lg - lg.max(-1, keepdims=True)))
        den = n.keysum(pu)
        pv_in = _r16(pu, 1024.0) if mutant == "p_fp16" else pu
        num = n.pv(pv_in, v)
        if mutant == "mask_finite" and per > 1:        # the next sample of the row tile masked with a finite value (sa_ref)
            i = np.arange(B)
            has = ((i % per != per - 1) & (i + 1 < B)).astype(F64)[:, None, None, None]
            w = math.exp(-10.0) * has
            num = num + w * v[np.minimum(i + 1, B - 1)].sum(-2, keepdims=True)
            den = den + w * L
        o = num / den
    if mutant == "heads_swapped":
        o = o[:, [1, 0, 3, 2]]
    return _store(n, o.transpose(0, 2, 1, 3).reshape(B, L, C))


def _affine(n, x, ab, mutant=None):
    if ab is None:
        return x
    C = x.shape[-1]
    ab = n.arr(ab)
    return x * ab[:, None, :C] + ab[:, None, C:]


def _straddle_ab(ab, B, L, TM):
    """mistake: every row of a TM-row tile takes the coefficients of the tile's first sample -> per-row coefficients [B L, 2C]"""
    rows = np.arange(B * L)
    return ab[(rows // TM * TM) // L].reshape(B, L, -1)


def _forward(n, W, x, ab=None, mutant=None, TM=0, stop=None, qkv_in=None, att_in=None):
    """The block over arithmetic n.  stop: 'qkv' | 'att' return that intermediate; qkv_in / att_in: start from a given one."""
    w = {k: n.arr(v) for k, v in W.items()} if W else {}
    x = n.arr(x) if x is not None else None
    B, L, C = (x if x is not None else qkv_in).shape[0], (x if x is not None else qkv_in).shape[1], \
        (x.shape[2] if x is not None else qkv_in.shape[2] // 3)
    xa = None
    if x is not None:
        if mutant == "straddle_first_coef" and ab is not None:
            abr = n.arr(_straddle_ab(np.asarray(ab), B, L, TM))
            xa = x * abr[..., :C] + abr[..., C:]
        elif mutant == "ab_after_ln":
            xa = x
        else:
            xa = _affine(n, x, ab)
    if att_in is None:
        if qkv_in is None:
            ln = _ln(n, xa, w["ln.weight"], w["ln.bias"])
            if mutant == "ab_after_ln":
                ln = _affine(n, ln, ab)
            qkv = _store(n, n.dot(ln, w["attention.in_proj_weight"]) + w["attention.in_proj_bias"])
        else:
            qkv = n.arr(qkv_in)
        if stop == "qkv":
            return qkv
        att = _attn(n, qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], mutant, per=(TM // L if TM and TM % L == 0 else 0))
    else:
        att = n.arr(att_in)
    if stop == "att":
        return att
    res = x if mutant == "resid_raw_x" else (_affine(n, x, ab) if mutant == "ab_after_ln" else xa)
    a = _store(n, n.dot(att, w["attention.out_proj.weight"]) + w["attention.out_proj.bias"] + res)
    f0 = _ln(n, a, w["ff_self.0.weight"], w["ff_self.0.bias"])
    f1 = n.dot(f0, w["ff_self.1.weight"]) + w["ff_self.1.bias"]
    g = n.dt(0.5) * f1 * (1 + n.erf(f1 * n.dt(math.sqrt(0.5))))
    return _store(n, n.dot(g, w["ff_self.3.weight"]) + w["ff_self.3.bias"] + a)


# ---- the input of a block: raw x, and its affine from memory (ab) or a recipe (FilmSpec) -----------------------------------------
def film_inputs(inp):
    """tests/stream_ops_ref.py's film_coef input of this case's FilmSpec"""
    f = inp["film"]
    return dict(B=inp["B"], C=inp["C"], HW=inp["L"], temb=f["temb"], t=f["t"], film=f["film"], gn=f["gn"], row_stats=False)


def coefficients(inp, dt=F64, mutant=None):
    """[B, 2C] = [A | B] of the block input, or None: ab as given, or film_coef's reference (imported, not restated)"""
    if inp.get("ab") is not None:
        return np.asarray(inp["ab"], dt)
    if inp.get("film") is None:
        return None
    fi = film_inputs(inp)
    if mutant == "t_of_sample0":
        return S.ref64("film_coef", fi, mutant="t_of_sample0")["ab"]
    if mutant == "gn_neighbour":
        fi = {**fi, "gn": {**fi["gn"], "stats": np.roll(fi["gn"]["stats"], 1, axis=0)}}
    return (S.ref64 if dt == F64 else S.ref32)("film_coef", fi)["ab"]


def crop_tokens(c, stride=None, lh=None, lw=None):
    stride = c["Wp"] if stride is None else stride
    lh, lw = (c["lh"] if lh is None else lh), (c["lw"] if lw is None else lw)
    return np.array([(lh + i) * stride + lw + j for i in range(c["H0"]) for j in range(c["D"])])


def crop_waves(L):
    return min(4, (L + 31) // 32)


def _block64(inp, x, ab):
    """sa_block_ref on the affine input of the samples x [b, L, C]: the reference and its bound"""
    xa = _affine(N64(), np.asarray(x, F64), ab)
    r = sa_block_ref(_sd(inp["W"]), "b", torch.from_numpy(xa.transpose(0, 2, 1)[..., None].copy()))
    cl = lambda z: z[..., 0].permute(0, 2, 1).numpy()
    merge = lambda z: z.permute(0, 2, 1, 3).reshape(z.shape[0], z.shape[2], -1).numpy()
    d = inp["C"] // HEADS
    return dict(out=cl(r["out"]), bound=cl(sa_bound(r)), q=merge(r["q"]) * math.sqrt(d), k=merge(r["k"]), v=merge(r["v"]),
                p=r["p"].numpy(), att=merge(r["p"] @ r["v"]), xa=xa)


def subset(inp):
    """the samples compared: all, or -- large B -- first, last, both sides of each boundary of the case and 8 seeded others"""
    B = inp["B"]
    if B <= 16:
        return np.arange(B)
    rng = np.random.default_rng(_seed("subset", inp["id"]))
    pick = {0, B - 1} | {b for e in inp.get("edges", ()) for b in (e - 1, e, e + 1) if 0 <= b < B} | set(rng.choice(B, 8, replace=False).tolist())
    return np.array(sorted(pick))


def _rows(v, sub):
    return None if v is None else np.asarray(v)[sub]


def ref64(op, inp, mutant=None):
    """{name: float64 array} of the compared samples (subset(inp)); 'bound' beside it for the whole-block launches"""
    sub = subset(inp)
    W, n = inp["W"], N64()
    if op == "core":
        qkv = inp["qkv"][sub]
        return {"out": _forward(n, None, None, qkv_in=qkv, stop="att", mutant=mutant)}
    ab = coefficients(inp, F64, mutant)
    x = inp["x"]
    if mutant == "walk_stuck":                             # a persistent walk that does not advance: sample i >= 256 gets i - 256's
        src = np.where(sub >= 256, sub - 256, sub)
        return {"out": _forward(n, W, x[src], _rows(ab, src))}
    xs, abs_ = x[sub], _rows(ab, sub)
    TM = 8192 // inp["C"]
    full = mutant in ("straddle_first_coef", "last_tile_dropped")       # these need every sample's row position
    if full:
        xs, abs_ = x, ab
    if op == "fused64":
        out = _forward(n, W, xs, abs_, mutant=mutant) if mutant else _block64(inp, xs, abs_)["out"]
        c = inp.get("crop")
        if c is None:
            return {"out": out}
        tok = crop_tokens(c, **({"stride": c["D"]} if mutant == "crop_stride_D" else {"lh": 0} if mutant == "lh_ignored"
                                 else {"lw": 0} if mutant == "lw_ignored" else {}))
        o = out[:, np.minimum(tok, inp["L"] - 1)]
        if mutant == "qw_last_dropped":                    # the last query of every wave's share is never written
            Q, nw = len(tok), crop_waves(inp["L"])
            qw = -(-Q // nw)
            o = o.copy()
            o[:, [min((w + 1) * qw, Q) - 1 for w in range(nw) if w * qw < Q]] = np.nan
        if inp.get("outc") is None:
            return {"out": o}
        w_, b_ = inp["outc"]
        return {"eps": (o @ w_.astype(F64) + (0.0 if mutant == "outc_bias_dropped" else F64(b_))).reshape(len(o), c["H0"], c["D"])}
    stop = {"qkv": "qkv", "head": "att", "tail": None}[op]
    if op == "tail":
        out = _forward(n, W, xs, abs_, mutant=mutant, TM=TM, att_in=inp["att"] if full else inp["att"][sub])
    else:
        out = _forward(n, W, xs, abs_, mutant=mutant, TM=TM, stop=stop)
    if mutant == "last_tile_dropped":
        out = out.copy().reshape(-1, out.shape[-1])
        out[len(out) // TM * TM:] = np.nan
        out = out.reshape(len(xs), inp["L"], -1)
    return {"out": out[sub] if full else out}


def _restate(n, op, inp):
    sub = subset(inp)
    if op == "core":
        return _forward(n, None, None, qkv_in=inp["qkv"][sub], stop="att")
    ab = coefficients(inp, n.dt if n.dt == F32 else F64)
    ab = None if ab is None else (ab.astype(F32) if n.dt == F32 else ab.astype(F32).astype(F64))     # the float32 the kernels hold
    kw = dict(att_in=inp["att"][sub]) if op == "tail" else dict(stop={"qkv": "qkv", "head": "att"}.get(op))
    return _forward(n, inp["W"], inp["x"][sub], _rows(ab, sub), **kw)


def ref32(op, inp):
    with np.errstate(under="ignore"):
        out = _restate(N32(), op, inp)
    assert out.dtype == F32
    return {"out": out.astype(F64)}


def ref_split(op, inp):
    return {"out": _restate(NSplit(), op, inp)}


def plain32(op, inp):
    """the admission evaluation: the op in float32 torch, its own sums"""
    sub = subset(inp)
    if op == "core":
        return {"out": _forward(_T32(), None, None, qkv_in=inp["qkv"][sub], stop="att").astype(F64)}
    ab = coefficients(inp, F32)
    kw = dict(att_in=inp["att"][sub]) if op == "tail" else dict(stop={"qkv": "qkv", "head": "att"}.get(op))
    out = _forward(_T32(), inp["W"], inp["x"][sub], _rows(ab, sub), **kw).astype(F64)
    c = inp.get("crop")
    if op != "fused64" or c is None:
        return {"out": out}
    o = out[:, crop_tokens(c)]
    if inp.get("outc") is None:
        return {"out": o}
    w_, b_ = inp["outc"]
    return {"eps": (o.astype(F32) @ w_ + F32(b_)).astype(F64).reshape(len(o), c["H0"], c["D"])}


class _T32(N64):
    """float32 with numpy's own (pairwise / BLAS) sums"""
    dt = F32


# ---- the scale of a partial op --------------------------------------------------------------------------------------------
def _ln_abs(v_abs, v, g, b):
    mu = v.mean(-1, keepdims=True)
    rs = 1 / np.sqrt(((v - mu) ** 2).mean(-1, keepdims=True) + EPS)
    return (v_abs + np.abs(mu)) * rs * np.abs(g) + np.abs(b), rs


def scale64(op, inp):
    """{'out': S_op} of a partial op (every term in absolute value) on the compared samples, and {'floor': ...}: the absolute floors
    of the split format where a lo half can be an fp16 subnormal (gemm_ref.floor_terms) -- 2^-29 per activation
    against |W| (*) 1 and 2^-32 per weight against 1 (*) |X| of the product that ends the launch (HEAD: of its v third, which the
    softmax only averages).  The floor is added to TAU_op S_op, never scaled by it."""
    def floor(x_abs, w):
        fw, fx = floor_terms(0, torch.from_numpy(x_abs.reshape(-1, x_abs.shape[-1])), torch.from_numpy(w), 1, 1, taps=1)
        return (2.0 ** -29 * fw.numpy() + 2.0 ** -32 * fx.numpy()).reshape(x_abs.shape[:-1] + (w.shape[0],))

    sub = subset(inp)
    W = {k: v.astype(F64) for k, v in inp["W"].items()} if inp.get("W") else {}
    n = N64()
    C, d = inp["C"], inp["C"] // HEADS

    def core_scale(q, k, v, v_abs, s_qk=None):
        B, L, _ = q.shape
        hd = lambda z: z.reshape(B, L, HEADS, d).transpose(0, 2, 1, 3)
        qh, kh = hd(q) / math.sqrt(d), hd(k)
        lg = qh @ np.swapaxes(kh, -1, -2)
        p = np.exp(lg - lg.max(-1, keepdims=True))
        p = p / p.sum(-1, keepdims=True)
        s = (np.abs(qh) @ np.swapaxes(np.abs(kh), -1, -2) if s_qk is None else s_qk).max(-1, keepdims=True)
        va = hd(v_abs)
        out = p @ va + s * va.max(-2, keepdims=True) / 1024.0
        return out.transpose(0, 2, 1, 3).reshape(B, L, C)

    if op == "core":
        qkv = inp["qkv"][sub].astype(F64)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        return {"out": core_scale(q, k, v, np.abs(v)), "floor": 0.0}
    ab = coefficients(inp, F64)
    x = inp["x"][sub].astype(F64)
    ab_s = _rows(ab, sub)
    xa = _affine(n, x, ab_s)
    xa_abs = np.abs(x) if ab is None else np.abs(x) * np.abs(ab_s[:, None, :C]) + np.abs(ab_s[:, None, C:])
    if op in ("qkv", "head"):
        ln_abs, rs = _ln_abs(xa_abs, xa, W["ln.weight"], W["ln.bias"])
        wi, bi = W["attention.in_proj_weight"], W["attention.in_proj_bias"]
        s_qkv = ln_abs @ np.abs(wi).T + np.abs(bi)
        fl = floor(ln_abs, wi)
        if op == "qkv":
            return {"out": s_qkv, "floor": fl}
        qkv = _forward(n, inp["W"], x, ab_s, stop="qkv")
        B, L = x.shape[:2]
        hd = lambda z: z.reshape(B, L, HEADS, d).transpose(0, 2, 1, 3)
        s_qk = hd(s_qkv[..., :C]) / math.sqrt(d) @ np.swapaxes(hd(s_qkv[..., C:2 * C]), -1, -2)
        return {"out": core_scale(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], s_qkv[..., 2 * C:], s_qk),
                "floor": np.broadcast_to(fl[..., 2 * C:].max(1, keepdims=True), x.shape).copy()}
    att = inp["att"][sub].astype(F64)
    wo = W["attention.out_proj.weight"]
    a = att @ wo.T + W["attention.out_proj.bias"] + xa
    a_abs = np.abs(att) @ np.abs(wo).T + np.abs(W["attention.out_proj.bias"]) + xa_abs
    f0_abs, _ = _ln_abs(a_abs, a, W["ff_self.0.weight"], W["ff_self.0.bias"])
    f1_abs = f0_abs @ np.abs(W["ff_self.1.weight"]).T + np.abs(W["ff_self.1.bias"])
    return {"out": 1.13 * f1_abs @ np.abs(W["ff_self.3.weight"]).T + np.abs(W["ff_self.3.bias"]) + a_abs,
            "floor": floor(1.13 * f1_abs, W["ff_self.3.weight"])}


def _both32(op, inp):
    """the worse of the two restatements, element by element, as one 'ref32' for train_ops_ref.tau"""
    r64 = ref64(op, inp)["out"]
    a, b = ref32(op, inp)["out"], ref_split(op, inp)["out"]
    return {"out": np.where(np.abs(a - r64) >= np.abs(b - r64), a, b)}


def tau(op, inp, r64=None, s64=None):
    """TAU_op by 8.15's rule and code, from the references alone"""
    return T.tau(op, inp, r64, s64, refs=(ref64, scale64, _both32, FLOOR_U))


def golden_tau(op, case_id):
    return json.load(open(GOLDEN))[f"{op}/{case_id}"] * U


def dot_tau(o64, w, b):
    """stream_ops_ref's out_step rule for eps = feat . w + b: 4 x the sequential float32 dot product's own error, floored"""
    s = np.abs(o64) @ np.abs(w.astype(F64)) + abs(float(b))
    r32 = (N32()._seq(o64.astype(F32), w.astype(F32)[None, :])[..., 0] + F32(b)).astype(F64)
    worst = float((np.abs(r32 - (o64.astype(F32).astype(F64) @ w.astype(F64) + float(b))) / s).max())
    return max(4 * worst, S.FLOOR_U["out_step"] * U), s


def bound(op, inp, tau_op=None):
    """{name: per-element bound} on the compared samples"""
    if op != "fused64":
        t = tau(op, inp) if tau_op is None else tau_op
        sc = scale64(op, inp)
        return {"out": t * sc["out"] + sc["floor"]}
    sub = subset(inp)
    r = _block64(inp, inp["x"][sub], _rows(coefficients(inp), sub))
    c = inp.get("crop")
    if c is None:
        return {"out": r["bound"]}
    tok = crop_tokens(c)
    bd, o = r["bound"][:, tok], r["out"][:, tok]
    if inp.get("outc") is None:
        return {"out": bd}
    w_, b_ = inp["outc"]
    td, s = dot_tau(o, w_, b_)
    return {"eps": (bd @ np.abs(w_.astype(F64)) + td * s).reshape(len(o), c["H0"], c["D"])}


def worst_ratio(got, ref, bd):
    worst = 0.0
    for k in ref:
        g = np.asarray(got[k], F64).reshape(ref[k].shape)
        err = np.abs(g - ref[k])
        r = np.where(err <= bd[k], err / np.maximum(bd[k], 1e-300), np.inf)
        r = np.where(np.isnan(ref[k]) & np.isnan(g), 0.0, r)
        worst = max(worst, float(r.max()))
    return worst


# ---- mutants ---------------------------------------------------------------------------------------------------------------
_SA6 = ("k_fp16", "q_fp16", "p_fp16", "v_fp16", "skip_rescale")
MUTANTS = {
    "fused64": ("ab_after_ln", "resid_raw_x", "t_of_sample0", "gn_neighbour", "crop_stride_D", "lh_ignored", "lw_ignored",
                "qw_last_dropped", "outc_bias_dropped", "key_tail_unmasked", "walk_stuck", "heads_swapped") + _SA6,
    "qkv": ("ab_after_ln", "t_of_sample0", "gn_neighbour", "last_tile_dropped", "straddle_first_coef"),
    "head": ("ab_after_ln", "heads_swapped", "mask_finite", "last_tile_dropped") + _SA6,
    "tail": ("resid_raw_x", "t_of_sample0", "gn_neighbour", "last_tile_dropped", "straddle_first_coef"),
    "core": ("heads_swapped", "key_tail_unmasked") + _SA6,
}


# ---- data ------------------------------------------------------------------------------------------------------------------
def _tokens(rng, fl, B, L, C):
    x = rng.standard_normal((B, L, C))
    if fl.startswith("mean"):                              # per-sample mean (the first LayerNorm sees offset tokens)
        x = x + float(fl[4:]) * np.where(np.arange(B) % 2, -1.0, 1.0)[:, None, None]
    elif fl == "chan5":
        x = x + 5 * rng.standard_normal(C)
    elif fl == "amp3":
        x = 3 * x
    elif fl == "scaled":                                   # per-sample scales 1 % apart: samples differ strongly across a long walk
        x = x * (1.01 ** (np.arange(B) % 16))[:, None, None]
    elif fl == "sparse":                                   # 2 % of the entries x 30, and a zero-variance row
        x = np.where(rng.random(x.shape) < 0.02, 30 * x, x)
        x[0, 0] = 0.75
    elif fl == "alt3":      # neighbouring samples 3 x apart: in a tile of several samples a key or value of the neighbour that leaks
        #                     into a query's softmax at any weight fp32 can see moves the output by far more than the bound
        x = x * np.where(np.arange(B) % 2, 3.0, 1.0)[:, None, None]
    return x.astype(F32)


def _ab(rng, B, C):
    return np.concatenate([1 + 0.3 * rng.standard_normal((B, C)), 0.3 * rng.standard_normal((B, C))], 1).astype(F32)


def _film(rng, x, t_count):
    """a FilmSpec on the raw x: a pending GroupNorm (partials that straddle samples where the shape allows), temb and film"""
    B, L, C = x.shape
    T_ = 7
    kind = "straddle" if B >= 3 and L >= 3 else "serial"
    gn = S._make_gn(rng, x, kind, "unit", "pos")
    t = np.array([T_ - 1] if t_count == 1 else [(3 * b + T_ - 1) % T_ for b in range(B)], np.int32)
    film = np.concatenate([1 + 0.2 * rng.standard_normal((B, C)), 0.2 * rng.standard_normal((B, C))], 1).astype(F32)
    return dict(gn=gn, temb=(0.3 * rng.standard_normal((T_, C))).astype(F32), t=t, T=T_, film=film)


def _core_qkv(rng, fl, B, L, C):
    """8.15's attention data on qkv directly, distinct per sample"""
    d = C // HEADS
    qkv = rng.standard_normal((B, L, 3 * C))
    if fl == "onehot":                                     # one key per query wins by a gap >= 32 logit units
        k = rng.standard_normal((B, L, HEADS, d))
        k /= np.linalg.norm(k, axis=-1, keepdims=True)
        pick = rng.integers(0, L, (B, L, HEADS))
        q = np.take_along_axis(k, pick[..., None].repeat(d, -1), 1) * 48 * math.sqrt(d)
        qkv[..., :C], qkv[..., C:2 * C] = q.reshape(B, L, C), k.reshape(B, L, C)
    elif fl == "tied" and L >= 2:
        qkv[:, 1, C:2 * C] = qkv[:, 0, C:2 * C]
        qkv[..., :C] *= 3
    elif fl == "equal":
        qkv[..., C:2 * C] = qkv[:, :1, C:2 * C]
    elif fl == "off1000":                                  # + 1000 in coordinate 0 of q and k of every head: the logits cancel it
        qkv[..., :2 * C:d] += 1000
        qkv[..., :2 * C] /= 32
    return qkv.astype(F32)


CORE_FLAVOURS = ("randn", "onehot", "tied", "equal", "off1000")
CROPS = {   # name: (H0, D, Wp, lh, lw, L)
    "h32": (32, 3, 8, 0, 2, 256), "h16": (16, 3, 8, 0, 2, 128), "q1": (1, 1, 8, 3, 5, 64), "cap256": (32, 4, 8, 0, 0, 256),
    "cap192": (16, 4, 8, 2, 3, 192), "ragged_qw": (5, 3, 8, 1, 1, 128), "l35": (4, 3, 8, 0, 2, 35), "l72": (8, 3, 8, 1, 2, 72),
}


def head_Ls(C):
    return [l for l in (1, 2, 4, 8, 16, 32, 64) if (8192 // C) % l == 0]


def straddle_B(L):
    """a batch whose rows exceed one tile and -- but for L = 64 -- leave a ragged last tile of 64 and of 32 rows.  Samples straddle
    tiles exactly where L does not divide the tile (8192 / C rows): L = 3, 5, 20, 48, 80 for both C.  L = 1 and 16 divide both
    tile sizes, so their tiles hold whole samples (several per tile, each row on its own sample's coefficients); L = 64 is a
    whole number of tiles per sample, the branch that loads the coefficients once per tile."""
    return {1: 67, 3: 23, 5: 15, 16: 5, 20: 5, 48: 3, 64: 3, 80: 3}[L]


def cases(op):
    """[(id, spec)]"""
    out = []
    if op == "fused64":
        # weak: 'onehot' is not admitted for this case (default_flavour has the measured ratios)
        data = {1: "randn", 5: "mean10", 32: "randn", 35: "mean50", 64: "randn", 128: "mean10", 192: "mean10", 256: "mean50",
                320: "randn", 512: "mean50"}
        for L in (1, 5, 32, 35, 64, 128, 192, 256, 320, 512):
            out.append((f"L{L}", dict(B=3, L=L, data=data[L], weak=L == 320)))
        for L in (5, 35, 64, 128, 256):
            out.append((f"L{L}_ab", dict(B=3, L=L, aff="ab", weak=L == 256)))
        for L, tc in ((35, 1), (128, 3), (256, 1), (256, 3)):
            out.append((f"L{L}_film_t{tc}", dict(B=3, L=L, aff="film", t_count=tc, weak=L == 256)))
        for L in (128, 256):
            out.append((f"L{L}_B300", dict(B=300, L=L, data="scaled", edges=(256,), weak=True)))
        out.append(("L128_mean300", dict(B=3, L=128, data="mean300")))
        out.append(("L64_chan5", dict(B=3, L=64, data="chan5")))
        out.append(("L35_amp3", dict(B=3, L=35, data="amp3", weak=True)))
        out.append(("L64_plain", dict(B=3, L=64, flavour="plain")))        # the one control: g = 1, a near-uniform softmax
        for name, c in CROPS.items():
            for outc in (0, 1):
                out.append((f"crop_{name}_outc{outc}", dict(B=3, L=c[5], crop=c[:5], outc=outc, weak=name == "h16",
                                                            aff=("ab" if name == "h16" else "film" if name == "l72" else None), t_count=3)))
        return out
    if op in ("qkv", "tail"):
        for C in (128, 256):
            for L in (1, 3, 5, 16, 20, 48, 64, 80):
                out.append((f"C{C}_L{L}_ab", dict(C=C, B=straddle_B(L), L=L, aff="ab", data=("sparse" if op == "qkv" and L in (5, 48) else "randn"))))
            for L, tc in ((3, 1), (5, 0), (20, 1), (48, 0), (64, 0)):
                B = straddle_B(L)
                out.append((f"C{C}_L{L}_film_t{tc or B}", dict(C=C, B=B, L=L, aff="film", t_count=tc or B)))
            out.append((f"C{C}_L16_plain", dict(C=C, B=5, L=16, flavour="plain", data="mean10")))
        return out
    if op == "head":
        for C in (128, 256):
            TM = 8192 // C
            for L in head_Ls(C):
                for B in sorted({1, TM // L, TM // L + 1}):
                    out.append((f"C{C}_L{L}_B{B}", dict(C=C, B=B, L=L, data="alt3", aff=("ab" if B == TM // L + 1 else None))))
            out.append((f"C{C}_L4_film", dict(C=C, B=TM // 4 + 1, L=4, aff="film", t_count=TM // 4 + 1)))
            out.append((f"C{C}_L8_sparse", dict(C=C, B=3, L=8, data="sparse")))
        return out
    for C in (64, 128, 256):
        for i, L in enumerate((1, 3, 4, 5, 12, 16, 20, 32)):
            out.append((f"d{C // 4}_L{L}_valu", dict(C=C, B=3, L=L, valu=1 if L == 32 else 0, data=CORE_FLAVOURS[(i + C // 64) % 5])))
        for i, L in enumerate((32, 48, 64, 80, 192, 256, 320, 512)):
            out.append((f"d{C // 4}_L{L}_mfma", dict(C=C, B=3, L=L, valu=0, data=CORE_FLAVOURS[(i + C // 128) % 5])))
        for L in (48, 80):
            out.append((f"d{C // 4}_L{L}_forced_valu", dict(C=C, B=3, L=L, valu=1, data="onehot")))
    return out


def core_lds(C, L, valu):
    """bytes of LDS launch_attention_auto asks for (csrc/attention.hip): beyond 160 KiB the launcher refuses"""
    d = C // HEADS
    if L >= 32 and not valu:
        Lp = (L + 31) // 32 * 32
        return (2 * Lp * (d + 8) + 2 * 32 * ((d + 31) // 32) * (Lp + 8)) * 2
    G = 64 // L if L <= 32 and L & (L - 1) == 0 else 1
    GS = L * (d + 4) + ((4 - (L * (d + 4)) % 64 + 64) % 64)
    return 2 * G * GS * 4


def default_flavour(op, c):
    """The strongest sharpening the admission condition allows: 'onehot' (g = 6), or for the cases marked weak 'moderate' (g = 4).
    ('onehot+widened' changes GroupNorm and cond_encoder weights only, no weight of a block: on a block's own weights it IS
    'onehot'; the offset tokens it stands for are the per-sample means of the data.)
    Measured on the CPU, worst element of float32 numpy against ref64 over the bound, 'onehot' / 'moderate':
      not admitted on 'onehot' (> ADMIT): L320 0.60 / 0.24 (0.47 .. 0.60 over the four admitted data kinds), L256_film_t1 0.59 / 0.23,
        L128_B300 0.57 / 0.28, L256_B300 0.69 / 0.34, crop_h16_outc0 0.51 / 0.19 (its outc1 twin shares the weights),
        L35_amp3 0.64 / 0.29 (amplitude x 3: 0.63 .. 0.86 on 'onehot' at L = 35, 64, 128);
      above 128 tokens 'onehot' crosses 0.5 from one seed or data kind to the next (L = 192: 0.31 .. 0.60, L = 512: 0.39 .. 0.84), so
        there a case keeps it only at 0.45 or less: L256_ab 0.50 / 0.25 and L256_film_t3 0.48 / 0.28 are weak too, while L192 0.31,
        L256 0.44, L512 0.39 and the crops at L = 192 / 256 (0.35 .. 0.41) stay on 'onehot';
      up to 128 tokens every other case is admitted on 'onehot', the closest L32 0.45, L35_film_t1 0.47, L128_film_t3 0.44."""
    if op != "fused64":
        return "onehot"
    return "moderate" if c.get("weak") else "onehot"


def make_inputs(op, case):
    cid, c = case
    rng = np.random.default_rng(_seed("sa_" + op, cid))
    C, B, L = c.get("C", 64), c["B"], c["L"]
    inp = dict(id=cid, op=op, C=C, B=B, L=L, edges=c.get("edges", ()), ab=None, film=None, crop=None, outc=None)
    if op == "core":
        inp.update(W=None, valu=c["valu"], qkv=_core_qkv(rng, c["data"], B, L, C), refused=core_lds(C, L, c["valu"]) > 160 * 1024)
        return inp
    inp["W"] = block_weights(C, c.get("flavour") or default_flavour(op, c))
    x = _tokens(rng, c.get("data", "randn"), B, L, C)
    if c.get("aff") == "film":
        x = (2 * x + 0.5).astype(F32)
        inp["film"] = _film(rng, x, c["t_count"])
    elif c.get("aff") == "ab":
        inp["ab"] = _ab(rng, B, C)
    inp["x"] = x
    if c.get("crop"):
        inp["crop"] = dict(zip(("H0", "D", "Wp", "lh", "lw"), c["crop"]))
        if c["outc"]:
            inp["outc"] = ((0.3 * rng.standard_normal(64)).astype(F32), 0.05)
    if op == "tail":                                       # the head outputs the block itself would hand over, as float32
        inp["att"] = _forward(N64(), inp["W"], x, coefficients(inp), stop="att").astype(F32)
    return inp


CHAINS = [(route, C) for route in ("qkv_core_tail", "head_tail") for C in (128, 256)]


def chain_inputs(route, C):
    """(first op, id, inputs) of a chain of launches, each fed the previous one's output: QKV -> CORE -> TAIL on samples that
    straddle tiles, HEAD -> TAIL on one full tile of whole samples plus one sample; the block input behind a FilmSpec"""
    TM = 8192 // C
    L, B = (20, 5) if route == "qkv_core_tail" else (16, TM // 16 + 1)
    first, cid = ("qkv" if route == "qkv_core_tail" else "head"), f"{route}_C{C}"
    return first, cid, make_inputs(first, (cid, dict(C=C, B=B, L=L, aff="film", t_count=B)))
