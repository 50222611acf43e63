"""One SelfAttention block in float64 with its intermediates, the weight flavours that make the softmax peaked, the
per-element tolerance of a block output and float64 models of kernel mistakes.  A plain module like tests/gemm_ref.py:
tests/test_sa_reference.py checks it on the CPU, tests/test_gpu_sa_fp64.py holds the HIP kernels against it.

Tolerance per output element:  TAU * A + TAU_S * SV.
  A   the block in absolute values after the softmax: P |v| through |W_o|, + |b_o| + |x| (residual); that error carried on
      through the second LayerNorm's Jacobian, |W_1|, GELU' <= 1.13 and |W_2|; plus the feed-forward's own products in
      absolute values.  It stands for a relative rounding error TAU in every stored value.
  SV  a relative error TAU_S in a logit.  S = max over keys of sum_d |q_d| |k_d| / sqrt d for the query and head, V = max over
      keys of |v| per channel of the head: p moves by at most p TAU_S S, the head output by at most 2 TAU_S S V (the 2 is
      inside TAU_S); carried through |W_o| and the feed-forward like A.
The constants were set from the first measured run on the MI355X; the table is in tests/test_gpu_sa_fp64.py.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

HEADS = 4
LOG2E = 1.4426950408889634
# block -> (input tap, output tap) of a debug handle / of the oracle's `taps`
BLOCKS = {"sa1": ("d1", "x2"), "sa2": ("d2", "x3"), "sa3": ("d3", "x4"), "sa4": ("u1", "a4"), "sa5": ("u2", "a5"),
          "sa6": ("u3", "a6")}
FLAVOURS = {"plain": (1.0, False), "moderate": (4.0, False), "onehot": (6.0, False), "onehot+widened": (6.0, True)}
MUTANTS = ("k_fp16", "q_fp16", "p_fp16", "v_fp16", "skip_rescale", "mask_finite")
COND = (3, 11)

# First measured run (MI355X, every route x flavour x geometry of tests/test_gpu_sa_fp64.py): the error follows A, hardly SV --
# max err / A is 6.0e-9 on 'plain' and 1.35e-8 on 'onehot' while SV grows 36 x -- so the S V term (no cancellation in q . k,
# max over keys) is a gross over-estimate and gets a small constant.  Worst err / (A + SV / 1024) = 1.25e-8: 2.8 x margin
# (not the full 4 x: a dropped p_lo in sa3, L = 4 and p ~ 1, where fp16 rounds P almost exactly, errs by only 1.1 x this bound).
TAU = 3.5e-8
TAU_S = TAU / 1024
_SD = {}


def sharpen(sd, g):
    """q and k rows of the six in_proj weights and biases x g: every logit x g^2."""
    out = {}
    for name, v in sd.items():
        v = torch.as_tensor(np.asarray(v)).clone().float()
        if name.endswith("attention.in_proj_weight") or name.endswith("attention.in_proj_bias"):
            v[: 2 * (v.shape[0] // 3)] *= g
        out[name] = v
    return out


def flavour_weights(flavour, cond_dim=COND[0] * COND[1], seed=21):
    """'plain' g = 1 (the control), 'moderate' g = 4, 'onehot' g = 6, 'onehot+widened' g = 6 on test_gpu_parity._widened
    (GroupNorm gains negative / zero, FiLM x 3: the first LayerNorm sees offset tokens)."""
    key = (flavour, cond_dim, seed)
    if key not in _SD:
        from state_policy_diffusionmodel_amd.weights import random_state_dict
        g, wide = FLAVOURS[flavour]
        base = random_state_dict(cond_dim, seed=seed, attention=True)
        if wide:
            from test_gpu_parity import _widened
            base = _widened(base, 5)
        _SD[key] = sharpen(base, g)
    return _SD[key]


def inputs(H, D, B):
    g = torch.Generator().manual_seed(1000 * H + 10 * D + B)
    x = torch.randn(B, 1, H, D, generator=g) * 1.5
    y = torch.randn(B, 1, *COND, generator=g)
    t = (torch.arange(B) * 37 + 5) % 1000                  # per-sample t
    return x, y, t


def head_tile_samples(c, n):
    """Samples in a row tile of sa_head_kernel (8192 / C rows of whole samples); 0 where it does not take the block."""
    tm = 8192 // c
    return tm // n if c in (128, 256) and tm % n == 0 else 0


def _r16(z, scale):
    return (z * scale).to(torch.float16).double() / scale


def _online(t2, v, skip_below):
    """Softmax-weighted sum over 32-key blocks with a running max, log2 units.  skip_below > 0 is the mistake: no rescale of
    the accumulated sum when the max rises by less than that."""
    m = torch.full(t2.shape[:-1] + (1,), -float("inf"), dtype=torch.float64)
    den = torch.zeros_like(m)
    acc = torch.zeros(t2.shape[:-1] + (v.shape[-1],), dtype=torch.float64)
    for j in range(0, t2.shape[-1], 32):
        blk = t2[..., j:j + 32]
        m_new = torch.maximum(m, blk.max(-1, keepdim=True).values)
        first = torch.isinf(m)
        alpha = torch.where(first, torch.zeros_like(m), torch.exp2(torch.where(first, torch.zeros_like(m), m - m_new)))
        alpha = torch.where(~first & (m_new - m < skip_below), torch.ones_like(alpha), alpha)
        p = torch.exp2(blk - m_new)
        den = den * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + p @ v[..., j:j + 32, :]
        m = m_new
    return acc / den


def sa_block_ref(sd, name, x, mutant=None, gap=30.0):
    """x (B, C, h, w) -> dict(out (B, C, h, w); q (with 1 / sqrt d), k, v (B, heads, L, d); logits, p (B, heads, L, L); and,
    without a mutant, A and SV (B, C, h, w)).  mutant: one of MUTANTS; gap: how far below the row max, in logit units,
    'mask_finite' puts each key of the next sample of the tile."""
    W = {k[len(name) + 1:]: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items() if k.startswith(name + ".")}
    x = x.double()
    b, c, hh, ww = x.shape
    n, d = hh * ww, c // HEADS
    heads = lambda z: z.reshape(b, n, HEADS, d).permute(0, 2, 1, 3)
    merge = lambda z: z.permute(0, 2, 1, 3).reshape(b, n, c)
    back = lambda z: z.transpose(1, 2).reshape(b, c, hh, ww)
    tok = x.reshape(b, c, n).transpose(1, 2)
    ln = F.layer_norm(tok, (c,), W["ln.weight"], W["ln.bias"], 1e-5)
    q, k, v = (heads(z) for z in F.linear(ln, W["attention.in_proj_weight"], W["attention.in_proj_bias"]).split(c, -1))
    q = q * (1.0 / math.sqrt(d))
    qm = _r16(q, 16.0) if mutant == "q_fp16" else q
    km = _r16(k, 16.0) if mutant == "k_fp16" else k
    vm = _r16(v, 16.0) if mutant == "v_fp16" else v
    logits = qm @ km.transpose(-1, -2)
    pu = torch.exp(logits - logits.max(-1, keepdim=True).values)
    den = pu.sum(-1, keepdim=True)
    p = pu / den
    if mutant == "p_fp16":
        o = (_r16(pu, 1024.0) @ vm) / den
    elif mutant == "skip_rescale":
        o = _online(logits * LOG2E, vm, 1.0)
    elif mutant == "mask_finite":
        per = head_tile_samples(c, n)
        i = torch.arange(b)
        has = ((i % per != per - 1) & (i + 1 < b)) if per > 1 else torch.zeros(b, dtype=torch.bool)
        w = math.exp(-gap) * has.double()[:, None, None, None]
        o = (pu @ vm + w * vm[(i + 1).clamp(max=b - 1)].sum(-2, keepdim=True)) / (den + w * n)
    else:
        o = p @ vm
    wo, bo = W["attention.out_proj.weight"], W["attention.out_proj.bias"]
    a = F.linear(merge(o), wo, bo) + tok
    g2 = W["ff_self.0.weight"]
    f0 = F.layer_norm(a, (c,), g2, W["ff_self.0.bias"], 1e-5)
    f1 = F.linear(f0, W["ff_self.1.weight"], W["ff_self.1.bias"])
    out = F.linear(F.gelu(f1), W["ff_self.3.weight"], W["ff_self.3.bias"]) + a
    res = dict(out=back(out), q=q, k=k, v=v, logits=logits, p=p)
    if mutant is None:
        sigma = (a.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
        hat = ((a - a.mean(-1, keepdim=True)) / sigma).abs()
        w1, w2 = W["ff_self.1.weight"].abs(), W["ff_self.3.weight"].abs()

        def carried(e):          # |d out| for |d a| <= e: directly, and through LayerNorm -> W_1 -> GELU -> W_2
            dln = g2.abs() / sigma * (e + e.mean(-1, keepdim=True) + hat * (hat * e).mean(-1, keepdim=True))
            return e + F.linear(1.13 * F.linear(dln, w1), w2)

        a_abs = F.linear(merge(p @ v.abs()), wo.abs(), bo.abs()) + tok.abs()
        ff_abs = F.linear(F.gelu(f1).abs() + 1.13 * F.linear(f0.abs(), w1, W["ff_self.1.bias"].abs()), w2,
                          W["ff_self.3.bias"].abs())
        s = (q.abs() @ k.abs().transpose(-1, -2)).max(-1, keepdim=True).values       # (B, heads, L, 1)
        vmax = v.abs().max(-2, keepdim=True).values                                   # (B, heads, 1, d)
        res["A"] = back(carried(a_abs) + ff_abs)
        res["SV"] = back(carried(F.linear(merge(s * vmax), wo.abs())))
    return res


def sa_bound(ref, tau=None, tau_s=None):
    return (TAU if tau is None else tau) * ref["A"] + (TAU_S if tau_s is None else tau_s) * ref["SV"]


def worst_ratio(got, ref, **kw):
    """max over elements of |got - out| / sa_bound."""
    return float(((got.double() - ref["out"]).abs() / sa_bound(ref, **kw)).max())


def softmax_stats(ref):
    """From the float64 reference: the largest logit range of a query, the median of max-p, and for blocks of more than 32
    keys the share of (sample, head, query) whose arg-max key is outside the first 32-key block and the rise of the running
    max after that block in log2 units."""
    lg, p = ref["logits"], ref["p"]
    st = dict(range=float((lg.max(-1).values - lg.min(-1).values).max()), median_max_p=float(p.max(-1).values.median()))
    if lg.shape[-1] > 32:
        st["argmax_outside"] = float((lg.argmax(-1) >= 32).double().mean())
        st["rise"] = (lg.max(-1).values - lg[..., :32].max(-1).values) * LOG2E
    return st
