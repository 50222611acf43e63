"""The CPU references of the training launches (tests/train_ops_ref.py) checked against themselves, without a GPU:
  1. ref64 equals float64 torch autograd of the corresponding torch expression to 1e-12 of the scale S, per element;
  2. every mutant of every op violates TAU * S on some element of some case of that op (a bound that cannot see a dropped
     row has no place in the GPU test);
  3. ref32 is within its own bound, TAU is finite (and zero exactly where equality is meant), and tests/golden/train_ops_tau.json
     holds the values the references produce.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_ops_tau.json")
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
_CACHE = {}


def case_data(op, case):
    """inputs, ref64, scale64 and TAU of a case, computed once"""
    key = (op, case[0])
    if key not in _CACHE:
        inp = R.make_inputs(op, case)
        r, s = R.ref64(op, inp), R.scale64(op, inp)
        _CACHE[key] = (inp, r, s, R.tau(op, inp, r, s))
    return _CACHE[key]


ALL = [(op, case) for op in R.OPS for case in R.cases(op)]
IDS = [f"{op}-{case[0]}" for op, case in ALL]


def _close(name, ref, want, scale, rel=1e-12):
    want = np.asarray(want.detach().numpy() if isinstance(want, torch.Tensor) else want, np.float64).reshape(ref.shape)
    # per element to 1e-12 of S; an element whose own S is tiny is held to 1e-14 of the output's largest value instead: torch
    # recomputes the statistics from x, and x - mean (x about 50, spread 0.5) costs it about a hundred float64 roundings
    floor = 1e-2 * float(np.abs(want).max()) if want.size else 0.0
    bad = ~(np.abs(ref - want) <= rel * np.maximum(np.maximum(scale, np.abs(want)), floor))
    assert not bad.any(), (name, int(bad.sum()), float(np.abs(ref - want).max()))


def _img(a, B, H, W):
    """channels-last rows [B H W][C] -> (B, C, H, W)"""
    return T64(a).reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def _rows(t):
    """(B, C, H, W) -> [B, H, W, C]"""
    return t.permute(0, 2, 3, 1).contiguous()


def _exact_stats(x, axis_rows):
    x = np.asarray(x, np.float64)
    mean = x.mean(axis_rows)
    var = ((x - np.expand_dims(mean, axis_rows)) ** 2).mean(axis_rows)
    return mean, 1 / np.sqrt(var + R.EPS)


def _autograd(op, inp):
    """{output name: float64 torch value} of the op's torch expression (inputs with float32-rounded statistics replaced by the
    exact ones are returned too)."""
    inp = dict(inp)
    if op in ("wgrad", "wgrad_mapped"):
        B, H, W, taps = inp["B"], inp["H"], inp["W"], inp["taps"]
        if op == "wgrad":
            dy, x = inp["dy"][:, :inp["Co"]], inp["x"][:, :inp["Ci"]]
        else:
            dy, x = inp["dy"][:, inp["pos_o"]], inp["x"][:, inp["pos_i"]]
        if taps == 1:
            w = torch.zeros(dy.shape[1], x.shape[1], dtype=torch.float64, requires_grad=True)
            F.linear(T64(x), w).backward(T64(dy))
        else:
            w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
            F.conv2d(_img(x, B, H, W), w, padding=1).backward(_img(dy, B, H, W))
        return inp, {"dst": w.grad}
    if op == "colsum":
        M, C, off = inp["M"], inp["C"], inp["off"]
        b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        F.linear(torch.zeros(M, 1, dtype=torch.float64), torch.zeros(C, 1, dtype=torch.float64), b).backward(T64(inp["buf"][:, off:off + C]))
        return inp, {"dst": b.grad}
    if op == "gn_stats":
        return inp, {}                                                         # checked through F.group_norm below
    if op in ("gn_bwd", "gn_bwd_mapped"):
        pos = inp["pos"]
        real = np.asarray(inp["y"], np.float64)[:, :, pos]
        B, HW, nr = real.shape
        inp["mean"], inp["rstd"] = _exact_stats(real.reshape(B, -1), 1)
        C = inp["y"].shape[2]
        dy, dgb = np.zeros((B, HW, C)), np.zeros((B, C, 2))
        for b in range(B):
            y = T64(real[b:b + 1]).permute(0, 2, 1).contiguous().requires_grad_()
            ga, be = T64(inp["gamma"][pos]).requires_grad_(), T64(inp["beta"][pos]).requires_grad_()
            out = F.group_norm(y, 1, ga, be, R.EPS)
            if inp["gelu"]:
                out = F.gelu(out)
            out.backward(T64(inp["g"][b:b + 1][:, :, pos]).permute(0, 2, 1))
            dy[b][:, pos] = y.grad[0].T.numpy()
            dgb[b, pos, 0], dgb[b, pos, 1] = ga.grad.numpy(), be.grad.numpy()
        return inp, {"dy": dy, "dgb": dgb}
    if op == "film_bwd":
        B = inp["z"].shape[0]
        t = np.asarray(inp["t"])
        z = T64(inp["z"]).requires_grad_()
        e = T64(inp["temb"])[torch.from_numpy(t if len(t) == B else np.repeat(t, B)).long()].clone().requires_grad_()
        if inp["film"] is None:
            (z + e[:, None, :]).backward(T64(inp["dout"]))
            return inp, {"dz": z.grad, "de": e.grad}
        film = T64(inp["film"]).requires_grad_()
        C = z.shape[2]
        (film[:, None, :C] * (z + e[:, None, :]) + film[:, None, C:]).backward(T64(inp["dout"]))
        return inp, {"dz": z.grad, "de": e.grad, "dfilm": film.grad}
    if op == "mse":
        lh, lw, H0, D = inp["lh"], inp["lw"], inp["H0"], inp["D"]
        e = T64(inp["eps_pad"]).requires_grad_()
        loss = F.mse_loss(e[:, lh:lh + H0, lw:lw + D], T64(inp["noise"]))
        loss.backward()
        out = {"loss": loss.reshape(1), "deps_pad": e.grad, "eps_out": e.detach()[:, lh:lh + H0, lw:lw + D]}
        if not inp.get("eps_out", 1):
            del out["eps_out"]
        return inp, out
    if op == "pool_bwd":
        x = T64(inp["in"]).permute(0, 3, 1, 2).contiguous().requires_grad_()
        F.max_pool2d(x, 2).backward(T64(inp["dout"]).permute(0, 3, 1, 2).contiguous())
        return inp, {"din": (T64(inp["din"]) + _rows(x.grad)).float().double()}      # one correctly rounded float32 add
    if op == "up_bwd":
        B, h, w, C = inp["B"], inp["h"], inp["w"], inp["C"]
        x = torch.zeros(B, C, h, w, dtype=torch.float64, requires_grad=True)
        F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True).backward(_img(inp["dcat"][:, :C], B, 2 * h, 2 * w))
        return inp, {"dx": T64(inp["dx"]) + _rows(x.grad)}
    if op in ("mish_bwd", "silu_bwd", "gelu_bwd"):
        x = T64(inp["u" if op == "gelu_bwd" else "cond"]).requires_grad_()
        if op == "mish_bwd":
            g, f, name = T64(inp["dm"][:, :, :x.shape[1]]).sum(0), F.mish, "grad_cond"
        elif op == "silu_bwd":
            g, f, name = T64(inp["ds"][:, :x.shape[1]]), F.silu, "grad_cond"
        else:
            g, f, name = T64(inp["dh"]), F.gelu, "du"
        f(x).backward(g)
        return inp, {name: x.grad}
    if op == "ln_fwd":
        x = T64(inp["x"])
        mean, rstd = _exact_stats(inp["x"], 1)
        return inp, {"y": F.layer_norm(x, (x.shape[1],), T64(inp["g"]), T64(inp["b"]), R.EPS), "mean": mean, "rstd": rstd}
    if op == "ln_bwd":
        inp["mean"], inp["rstd"] = _exact_stats(inp["x"], 1)
        rows, C = inp["x"].shape
        x = T64(inp["x"]).requires_grad_()
        part = np.zeros((R.ln_bwd_blocks(rows), 2 * C))
        for k in range(part.shape[0]):                                         # the affine gradients of each 64-row block
            ga, be = T64(inp["gamma"]).requires_grad_(), torch.zeros(C, dtype=torch.float64, requires_grad=True)
            sl = slice(k * R.LN_BWD_ROWS, min(rows, (k + 1) * R.LN_BWD_ROWS))
            F.layer_norm(x[sl], (C,), ga, be, R.EPS).backward(T64(inp["gy"][sl]))
            part[k, :C], part[k, C:] = ga.grad.numpy(), be.grad.numpy()
        dx = x.grad if inp["add"] is None else x.grad + T64(inp["add"])
        return inp, {"dx": dx, "part": part}
    if op in ("attn_fwd_lse", "attn_bwd"):
        B, L, C, heads = inp["B"], inp["L"], inp["C"], inp["heads"]
        d = C // heads
        q, k, v = (t.contiguous().requires_grad_() for t in T64(inp["qkv"]).reshape(B, L, 3, heads, d).permute(2, 0, 3, 1, 4))
        out = F.scaled_dot_product_attention(q, k, v)
        flat = lambda t: t.permute(0, 2, 1, 3).reshape(B, L, C)
        lse = torch.logsumexp(q @ k.transpose(-1, -2) / d ** 0.5, -1)
        if op == "attn_fwd_lse":
            return inp, {"out": flat(out), "lse": lse}
        inp["out"], inp["lse"] = flat(out).detach().numpy(), lse.detach().numpy()      # the exact forward, not its float32 rounding
        out.backward(T64(inp["dout"]).reshape(B, L, heads, d).permute(0, 2, 1, 3))
        return inp, {"dqkv": torch.stack([q.grad, k.grad, v.grad], 0).permute(1, 3, 0, 2, 4).reshape(B, L, 3 * C)}
    if op == "simple_tail_bwd":
        B, HW, Co, Cr, Cz = (inp[k] for k in ("B", "HW", "Co", "Cr", "Cz"))
        z = torch.zeros(B, HW, Cz, dtype=torch.float64, requires_grad=True)
        temb = torch.zeros(B, Cr, dtype=torch.float64, requires_grad=True)
        cemb = torch.zeros(B, 32, dtype=torch.float64, requires_grad=True)
        out = torch.cat([z[:, :, :Cr] + temb[:, None, :], cemb[:, None, :].expand(B, HW, 32),
                         torch.zeros(B, HW, Co - Cr - 32, dtype=torch.float64)], 2)
        out.backward(T64(inp["dout"]))
        return inp, {"dz": z.grad, "dtemb": temb.grad, "dcemb": cemb.grad}
    raise KeyError(op)


@pytest.mark.parametrize("op,case", ALL, ids=IDS)
def test_ref64_equals_torch_autograd(op, case):
    inp, want = _autograd(op, R.make_inputs(op, case))
    got, scale = R.ref64(op, inp), R.scale64(op, inp)
    if op == "gn_stats":                                                       # (y - mean) rstd is F.group_norm of the real lanes
        real = T64(inp["y"][:, :, inp["pos"]]).permute(0, 2, 1).contiguous()
        norm = F.group_norm(real, 1, eps=R.EPS).numpy()
        mine = (real.numpy() - got["mean"][:, None, None]) * got["rstd"][:, None, None]
        assert np.abs(mine - norm).max() <= 1e-12 * max(1.0, np.abs(norm).max() * float(got["rstd"].max()))
        return
    assert set(want) == set(got)
    for name in got:
        assert np.isfinite(got[name]).all(), name
        # (peaked attention: two float64 evaluations of exp(s - lse) at |s| about 1100 already differ by |s| 2^-53 times a few
        # roundings, 1e-12 of P)
        _close(name, got[name], want[name], scale[name], 1e-10 if case[1]["flavour"] == "peaked" else 1e-12)


@pytest.mark.parametrize("op", R.OPS)
def test_every_mutant_violates_the_bound(op):
    caught = {m: [] for m in R.MUTANTS[op]}
    for case in R.cases(op):
        inp, r, s, t = case_data(op, case)
        for m in caught:
            if R.worst_ratio(R.ref64(op, inp, mutant=m), r, s, t) > 1:
                caught[m].append(case[0])
    assert R.MUTANTS[op], op
    assert all(caught.values()), {m: c for m, c in caught.items() if not c}


@pytest.mark.parametrize("op,case", ALL, ids=IDS)
def test_ref32_is_within_its_own_bound(op, case):
    inp, r, s, t = case_data(op, case)
    assert np.isfinite(t) and t >= 0
    assert R.worst_ratio(R.ref32(op, inp), r, s, t) <= 0.25 + 1e-9 or t == 0   # TAU is 4 x its worst error (or the floor above it)
    if t == 0:                                                                 # equality is meant: nothing rounds, or all is zero
        assert R.worst_ratio(R.ref32(op, inp), r, s, t) == 0
        assert op == "pool_bwd" or case[1]["flavour"] == "zero" or (op, case[0]) == ("colsum", "M1"), (op, case[0])
    else:
        assert t >= R.FLOOR_U.get(op, 0) * R.U
        # the widest are the attention backward's rows under a score offset of +1000: 4 x (64 sequential roundings at 1000 u)
        assert t < 4e-3, "a bound this wide checks nothing"
    if case[1]["flavour"] == "zero" and op != "mse":                           # a zero gradient gives exact zeros
        for name, v in r.items():
            if op in ("pool_bwd", "up_bwd"):                                   # ... added to what was there
                assert np.array_equal(v, np.asarray(inp["din" if op == "pool_bwd" else "dx"], np.float64).reshape(v.shape))
            elif (op, name) != ("ln_bwd", "dx") or inp["add"] is None:
                assert not v.any(), name


def _tau_table():
    table = {}
    for op, case in ALL:
        table.setdefault(op, {})[case[0]] = float(f"{case_data(op, case)[3]:.6e}")
    return table


def test_golden_tau_table_is_current():
    table = _tau_table()
    if os.environ.get("SPDM_WRITE_GOLDEN") == "1":
        with open(GOLDEN, "w") as fh:
            json.dump(table, fh, indent=1, sort_keys=True)
            fh.write("\n")
    with open(GOLDEN) as fh:
        assert json.load(fh) == table


def test_weight_gradient_cases_hit_their_geometry():
    """the chunk counts and rows per chunk the case table names are what the row-split rule gives"""
    for op in ("wgrad", "wgrad_mapped"):
        for cid, kw in R.cases(op):
            M = kw["B"] * kw["H"] * kw["W"]
            assert R.wgrad_geometry(M, kw["taps"], kw["Co"], kw["Ci"]) == kw["geom"], cid
    n, rows = R.wgrad_geometry(1409, 1, 64, 64)
    assert (n, rows) == (22, 68) and 21 * rows >= 1409 and 1409 - 20 * rows == 49      # an empty last chunk, a ragged 49 before it
    assert [R.ln_bwd_blocks(r) for r in (1, 5, 64, 65, 130)] == [1, 1, 1, 2, 3]
