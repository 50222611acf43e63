"""The CPU references of the encoder / decoder launches (tests/frame_ops_ref.py) checked against themselves, without a GPU:
  1. ref64 of every op equals float64 torch (F.conv2d, F.conv_transpose2d, F.linear, autograd) to 1e-12 of the scale S;
  2. the chain of op references reproduces autoencoder_ref.decoder_grads and encoder_train_ref.encoder_grads;
  3. every mutant of every op violates TAU * S on some element of some case of that op; `sq` summed in float32 violates its own;
  4. ref32 is within its own bound and tests/golden/frame_ops_tau.json holds the values the references produce;
  5. on the chosen seeds every pre-activation a kink kernel decides exceeds 2^-40 of its S, so that numpy's and the device's
     float64 sums cannot disagree on a sign; the kink references obey the rule the GPU test states.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frame_ops_ref as R
from autoencoder_ref import decoder_grads
from encoder_train_ref import encoder_grads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_ops_tau.json")
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
_CACHE = {}


def case_data(op, case):
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
    bad = ~(np.abs(ref - want) <= rel * np.maximum(scale, np.abs(want)))
    assert not bad.any(), (name, int(bad.sum()), float(np.abs(ref - want).max()))


def _dec_torch_weights(inp):
    """kernel layout [ci][kk][co] -> torch's (ci, co, 2, 2)"""
    out = {}
    for k, (ci, co) in (("2", (64, 32)), ("4", (32, 16)), ("6", (16, 3))):
        if "w" + k in inp:
            out["w" + k] = T64(np.asarray(inp["w" + k]).reshape(ci, 2, 2, co)).permute(0, 3, 1, 2).contiguous()
    return out


def _relu_grad(saved, upstream):
    """(saved > 0) upstream by autograd through F.relu: torch's convention at +0.0, -0.0 and subnormals"""
    x = T64(np.asarray(saved, np.float32)).requires_grad_()
    F.relu(x).backward(T64(upstream))
    return x.grad


def _torch(op, inp):
    if op in ("enc_kinks", "dec_kinks", "dec_unperm_conv", "dec_unperm_linear"):
        return None
    if op.startswith("enc"):
        n = inp["n"]
        img, w1, b1, w2, b2, w3, b3 = (T64(inp[k]) for k in ("img", "w1", "b1", "w2", "b2", "w3", "b3"))
        a1 = F.relu(F.conv2d(img, w1, b1, stride=2, padding=1))
        a2 = F.relu(F.conv2d(a1, w2, b2, stride=2))
        x3 = a2.reshape(n, 32, 12, 2, 12, 2).permute(0, 2, 4, 1, 3, 5).reshape(n * 144, 128)
        if op == "enc_convs":
            out = {"feat": F.relu(F.conv2d(a2, w3, b3, stride=2)).flatten(1)}
            if inp["train"]:
                out["x3"] = x3
            return out
        if op == "enc_x2":
            v = a1[:, :, :48, :48].reshape(n, 16, 12, 2, 2, 12, 2, 2).permute(0, 2, 5, 3, 6, 1, 4, 7)
            return {"x2": v.reshape(n * 576, 64)}
        if op == "enc_dz3":
            return {"dz3": _relu_grad(inp["feat"], inp["dfeat"]).reshape(n, 64, 144).permute(0, 2, 1).reshape(n * 144, 64)}
        if op == "enc_dz2":
            return {"dz2": _relu_grad(inp["x3"], inp["dx3"]).reshape(n * 144, 32, 4).permute(0, 2, 1).reshape(n * 144, 128)}
        if op == "enc_conv1_wgrad":
            g = _relu_grad(inp["x2"], inp["dx2"]).reshape(n, 12, 12, 2, 2, 16, 2, 2)        # n qy qx kyq kxq c1 ky kx
            g = g.permute(0, 5, 1, 3, 6, 2, 4, 7).reshape(n, 16, 48, 48)
            G = torch.zeros(n, 16, 49, 49, dtype=torch.float64)
            G[:, :, :48, :48] = g
            w, b = w1.clone().requires_grad_(), b1.clone().requires_grad_()
            F.conv2d(img, w, b, stride=2, padding=1).backward(G)
            return {"dw": w.grad.reshape(192), "db": b.grad}
    if op == "add":
        return {"dst": (torch.from_numpy(inp["dst"]) + torch.from_numpy(inp["src"])).double()}
    W = _dec_torch_weights(inp)
    n = inp.get("n", 0)
    if op == "dec_convs":
        h0 = T64(inp["h0"]).reshape(n, 12, 12, 64).permute(0, 3, 1, 2)
        a1 = F.relu(F.conv_transpose2d(h0, W["w2"], T64(inp["b2"]), stride=2))
        a2 = F.relu(F.conv_transpose2d(a1, W["w4"], T64(inp["b4"]), stride=2))
        out = {"recon": torch.sigmoid(F.conv_transpose2d(a2, W["w6"], T64(inp["b6"]), stride=2))}
        if inp["train"]:
            out["a1"], out["a2"] = R.nchw_to_rows(a1.numpy(), 1), R.nchw_to_rows(a2.numpy(), 2)
        return out
    if op == "dec_bwd6":
        r, t = T64(inp["recon"]), T64(inp["target"])
        dz6 = float(inp["scale"]) * (r - t) * r * (1 - r)
        x = T64(R.rows_to_nchw(np.asarray(inp["a2"], np.float32), n, 2)).requires_grad_()
        w = T64(np.asarray(inp["w6"]).reshape(16, 2, 2, 3)).permute(0, 3, 1, 2).contiguous().requires_grad_()
        b = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(F.relu(x), w, b, stride=2).backward(dz6)
        return {"dz4": R.nchw_to_rows(x.grad.numpy(), 2), "dw": w.grad.reshape(192), "db": b.grad}
    if op == "dec_dgrad4":
        x = T64(R.rows_to_nchw(np.asarray(inp["a1"], np.float32), n, 1)).requires_grad_()
        w = T64(np.asarray(inp["w4"]).reshape(32, 2, 2, 16)).permute(0, 3, 1, 2).contiguous()
        g = R.rows_to_nchw(np.asarray(inp["dz4"], np.float64).reshape(-1, 16), n, 2)
        F.conv_transpose2d(F.relu(x), w, None, stride=2).backward(T64(g))
        return {"dz2": R.nchw_to_rows(x.grad.numpy(), 1)}
    if op == "dec_colsum":
        s = T64(inp["src"]).sum(0)
        if inp["fold"] == 1:
            return {"dst": s.reshape(144, 64).t().reshape(-1)}
        return {"dst": s.reshape(4, -1).sum(0)}
    if op == "dec_loss":
        return {"loss": T64(inp["sq"]).sum().reshape(1) / (inp["n"] * 27648.0)}
    if op == "frame_wgrad":
        w = torch.zeros(inp["dy"].shape[1], inp["x"].shape[1], dtype=torch.float64, requires_grad=True)
        F.linear(T64(inp["x"]), w).backward(T64(inp["dy"]))
        return {"dst": w.grad}
    return None


@pytest.mark.parametrize("op,case", ALL, ids=IDS)
def test_ref64_equals_float64_torch(op, case):
    inp, got, scale, _ = case_data(op, case)
    want = _torch(op, inp)
    if want is None:
        assert op in ("enc_kinks", "dec_kinks", "dec_unperm_conv", "dec_unperm_linear")      # held below
        return
    assert set(want) == set(got)
    for name in got:
        assert np.isfinite(got[name]).all(), name
        _close(name, got[name], want[name], scale[name])


def test_unperm_inverts_the_kernel_layout():
    rng = np.random.default_rng(5)
    sd = R.dec_state(rng)
    K = R.dec_kernel_layout(sd)
    for k, (ci, co) in (("2", (64, 32)), ("4", (32, 16)), ("6", (16, 3))):
        got = R.exact32("dec_unperm_conv", {"src": K["w" + k].ravel(), "cin": ci, "cout": co})["dst"]
        assert np.array_equal(got, sd[k + ".weight"].ravel())
    assert np.array_equal(R.exact32("dec_unperm_linear", {"src": K["w0"].ravel()})["dst"], sd["0.weight"].ravel())
    assert np.array_equal(R.ref64("dec_colsum", {"src": K["b0"][None, :], "M": 1, "C": 9216, "fold": 1})["dst"], sd["0.bias"])


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)), float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("flavour", ["init", "trained120", "dead"])
def test_chain_of_decoder_ops_reproduces_decoder_grads(flavour):
    n = 2
    rng = np.random.default_rng(11)
    K, lat, f, target = R.dec_world(rng, n, flavour)
    sd = {"0.weight": K["w0"].reshape(144, 64, 128).transpose(1, 0, 2).reshape(9216, 128), "0.bias": K["b0"].reshape(144, 64).T.ravel()}
    for k, (ci, co) in (("2", (64, 32)), ("4", (32, 16)), ("6", (16, 3))):
        sd[k + ".weight"], sd[k + ".bias"] = K["w" + k].reshape(ci, 2, 2, co).transpose(0, 3, 1, 2), K["b" + k]
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
    loss, grads, glat = decoder_grads(sd, torch.from_numpy(lat), torch.from_numpy(target))
    D = np.float64
    h0 = (lat.astype(D) @ K["w0"].astype(D).T + K["b0"]).reshape(-1, 64)
    fw = R.ref64("dec_convs", dict(K, h0=h0, train=1))
    sq = ((fw["recon"] - target) ** 2).reshape(n, -1).sum(1)
    assert abs(R.ref64("dec_loss", {"sq": sq, "n": n})["loss"][0] - loss) <= 1e-13 * loss
    b6 = R.ref64("dec_bwd6", {"recon": fw["recon"], "target": target, "a2": fw["a2"], "w6": K["w6"], "scale": 2.0 / (n * R.PIX)})
    unperm = lambda src, ci, co: src.reshape(ci, 4, co).transpose(0, 2, 1).ravel()
    dz4 = b6["dz4"].reshape(-1, 64)
    g4 = R.ref64("frame_wgrad", {"dy": fw["a1"], "x": dz4, "M": n * 576, "which": 3})["dst"]
    d4 = R.ref64("dec_dgrad4", {"dz4": dz4, "a1": fw["a1"], "w4": K["w4"]})["dz2"]
    dz2 = d4.reshape(-1, 128)
    g2 = R.ref64("frame_wgrad", {"dy": h0, "x": dz2, "M": n * 144, "which": 4})["dst"]
    dh0 = (dz2 @ K["w2"].astype(D).reshape(64, 128).T).reshape(n, 9216)
    g0 = R.ref64("frame_wgrad", {"dy": dh0, "x": lat, "M": n, "which": 5})["dst"]
    mine = {"6.weight": b6["dw"], "6.bias": b6["db"], "4.weight": unperm(g4, 32, 16),
            "4.bias": R.ref64("dec_colsum", {"src": dz4, "M": n * 576, "C": 64, "fold": 4})["dst"],
            "2.weight": unperm(g2, 64, 32), "2.bias": R.ref64("dec_colsum", {"src": dz2, "M": n * 144, "C": 128, "fold": 4})["dst"],
            "0.weight": g0.reshape(144, 64, 128).transpose(1, 0, 2).ravel(),
            "0.bias": R.ref64("dec_colsum", {"src": dh0, "M": n, "C": 9216, "fold": 1})["dst"]}
    for k, g in mine.items():
        assert max(_rel(g, grads[k].numpy())) <= 1e-11, (k, _rel(g, grads[k].numpy()))
    assert max(_rel(dh0 @ K["w0"].astype(D), glat.numpy())) <= 1e-11


@pytest.mark.parametrize("flavour", ["init", "trained", "dead"])
def test_chain_of_encoder_ops_reproduces_encoder_grads(flavour):
    n = 2
    rng = np.random.default_rng(13)
    inp = R._enc_inputs(rng, flavour, n)
    w7 = (rng.standard_normal((128, 9216)) / 96).astype(np.float32)
    g = rng.standard_normal((n, 128)).astype(np.float32)
    sd = {"0.weight": inp["w1"], "0.bias": inp["b1"], "2.weight": inp["w2"], "2.bias": inp["b2"], "4.weight": inp["w3"],
          "4.bias": inp["b3"], "7.weight": w7, "7.bias": np.zeros(128, np.float32)}
    _, grads = encoder_grads({k: torch.from_numpy(v) for k, v in sd.items()}, torch.from_numpy(inp["img"]), torch.from_numpy(g))
    D = np.float64
    fw = R.ref64("enc_convs", inp)
    dfeat = g.astype(D) @ w7.astype(D)
    # (the masked permutations in float64 here: their references store float32; held to the same order below)
    dz3 = np.where(fw["feat"].reshape(n, 64, 144).transpose(0, 2, 1).reshape(-1, 64) > 0,
                   dfeat.reshape(n, 64, 144).transpose(0, 2, 1).reshape(-1, 64), 0)
    g3 = R.ref64("frame_wgrad", {"dy": dz3, "x": fw["x3"], "M": n * 144, "which": 1})["dst"]
    dx3 = dz3 @ inp["w3"].astype(D).reshape(64, 128)
    dz2 = np.where(fw["x3"] > 0, dx3, 0).reshape(-1, 32, 4).transpose(0, 2, 1).reshape(-1, 32)
    # the float32 permutation reference moves the same elements to the same places
    p32 = R.exact32("enc_dz2", {"x3": fw["x3"].astype(np.float32), "dx3": dx3.astype(np.float32)})["dz2"]
    assert np.array_equal(p32.reshape(-1, 32), np.where(fw["x3"].astype(np.float32) > 0, dx3.astype(np.float32), np.float32(0))
                          .reshape(-1, 32, 4).transpose(0, 2, 1).reshape(-1, 32))
    x2 = R.ref64("enc_x2", inp)["x2"]
    g2 = R.ref64("frame_wgrad", {"dy": dz2, "x": x2, "M": n * 576, "which": 2})["dst"]
    dx2 = dz2 @ inp["w2"].astype(D).reshape(32, 64)
    c1 = R.ref64("enc_conv1_wgrad", dict(inp, x2=x2, dx2=dx2))
    mine = {"4.weight": g3, "4.bias": dz3.sum(0), "2.weight": g2, "2.bias": dz2.sum(0), "0.weight": c1["dw"], "0.bias": c1["db"]}
    for k, v in mine.items():
        assert max(_rel(v, grads[k].numpy())) <= 1e-11, (k, _rel(v, grads[k].numpy()))
    assert np.array_equal(R.exact32("enc_dz3", {"feat": fw["feat"].astype(np.float32), "dfeat": dfeat.astype(np.float32)})["dz3"],
                          np.where(fw["feat"].astype(np.float32) > 0, dfeat.astype(np.float32), np.float32(0))
                          .reshape(n, 64, 144).transpose(0, 2, 1).reshape(-1, 64))


@pytest.mark.parametrize("op", R.OPS)
def test_every_mutant_violates_the_bound(op):
    caught = {m: [] for m in R.MUTANTS[op]}
    for case in R.cases(op):
        inp, r, s, t = case_data(op, case)
        for m in caught:
            if R.worst_ratio(R.ref64(op, inp, mutant=m), r, s, t) > 1:
                caught[m].append(case[0])
    assert R.MUTANTS[op] or op in ("enc_kinks", "dec_kinks"), op
    assert all(caught.values()), {m: c for m, c in caught.items() if not c}


def _sq_cases():
    return [c for c in R.cases("dec_convs") if c[1]["train"]]


@pytest.mark.parametrize("case", _sq_cases(), ids=[c[0] for c in _sq_cases()])
def test_sq_in_float32_violates_its_bound(case):
    inp, r, _, _ = case_data("dec_convs", case)
    recon32 = r["recon"].astype(np.float32)
    ref, S, model = R.sq_refs(recon32, inp["target"])
    t = R.sq_tau(ref, S, model)
    assert 0 < t < 1e-8, t                                                     # far inside float32: a float64 quantity
    assert (np.abs(model - ref) <= 0.25 * t * S + 1e-300).all()
    bad = R.sq_refs(recon32, inp["target"], mutant="sum_in_float32")[2]
    assert (np.abs(bad - ref) > t * S).any()


@pytest.mark.parametrize("op,case", ALL, ids=IDS)
def test_ref32_is_within_its_own_bound(op, case):
    inp, r, s, t = case_data(op, case)
    assert np.isfinite(t) and t >= 0
    ratio = R.worst_ratio(R.ref32(op, inp), r, s, t)
    assert ratio <= 0.25 + 1e-9 or t == 0
    fl = case[1]["flavour"]
    if op in R.EXACT:                                                          # equality is meant: nothing rounds
        assert t == 0 and ratio == 0
        assert all(not v.any() for v in s.values())
    elif t == 0:                                                               # nothing rounded on this data: equality is the bound
        assert ratio == 0
        assert fl in ("zero", "alldead", "a1dead") or (op, case[1].get("M"), case[1].get("fold")) == ("dec_colsum", 1, 1), (op, case[0])
    else:
        assert t >= R.FLOOR_U.get(op, 0) * R.U
        assert t < 1e-3, "a bound this wide checks nothing"
    if fl == "zero":                                                           # a zero gradient gives exact zeros
        assert all(not v.any() for v in r.values())
    if (op, fl) == ("enc_dz2", "alldead") or (op, fl) == ("dec_dgrad4", "a1dead"):      # every unit of the layer off
        assert not r["dz2"].any() and not inp["x3" if op == "enc_dz2" else "a1"].any()
    if (op, fl) == ("dec_bwd6", "a2dead"):
        assert not r["dz4"].any() and not r["dw"].any() and r["db"].all() and not inp["a2"].any()


def _tau_table():
    table = {}
    for op, case in ALL:
        table.setdefault(op, {})[case[0]] = float(f"{case_data(op, case)[3]:.6e}")
    for case in _sq_cases():
        inp, r, _, _ = case_data("dec_convs", case)
        table.setdefault("dec_convs_sq", {})[case[0]] = float(f"{R.sq_tau(*R.sq_refs(r['recon'].astype(np.float32), inp['target'])):.6e}")
    return table


def test_golden_tau_table_is_current():
    table = _tau_table()
    if os.environ.get("SPDM_WRITE_GOLDEN") == "1":
        with open(GOLDEN, "w") as fh:
            json.dump(table, fh, indent=1, sort_keys=True)
            fh.write("\n")
    with open(GOLDEN) as fh:
        assert json.load(fh) == table


KINK_CASES = [(op, c) for op in ("enc_kinks", "dec_kinks", "enc_x2") for c in R.cases(op)]


@pytest.mark.parametrize("op,case", KINK_CASES, ids=[f"{o}-{c[0]}" for o, c in KINK_CASES])
def test_kink_margin_and_rule(op, case):
    inp = case_data(op, case)[0]
    assert R.kink_margin(op, inp) > 2.0 ** -40                                 # no float64 sum can land on the other side
    if op == "enc_x2":
        return
    want = R.exact32(op, inp)
    names = ("feat", "x3") if op == "enc_kinks" else ("a1", "a2")
    changed = 0
    for k in names:
        a32, out = np.asarray(inp[k], np.float32).reshape(want[k].shape), want[k]
        kept = out.view(np.uint32) == a32.view(np.uint32)
        assert set(np.unique(out[~kept]).tolist()) <= {0.0, float(R.KINK)}
        assert (a32[~kept & (out == 0)] > 0).all() and (a32[~kept & (out > 0)] <= 0).all()
        changed += int((~kept).sum())
    if case[1]["saved"] in ("ones", "neg"):                                    # a kernel that leaves the map alone is seen
        assert changed > 0


def test_geometry_restatements_and_cases_hit_their_edges():
    assert R.colsum_geometry(16384) == (64, 256) and R.colsum_geometry(16385) == (68, 241) and R.colsum_geometry(1) == (64, 1)
    assert R.colsum_geometry(65) == (64, 2) and R.colsum_geometry(63) == (64, 1)
    assert [R.conv1_wgrad_blocks(n) for n in (1, 2, 3, 5)] == [1, 2, 2, 3] and 2 * 576 - 1024 == 128
    # the 256-slab cap of the decoder's thin layers against the encoder's budget, from 29 frames up
    assert R.frame_wgrad_geometry(576 * 28, 3) == R.frame_wgrad_geometry(576 * 28, 2) == (252, 64)
    assert R.frame_wgrad_geometry(576 * 29, 3) == (256, 68) and R.frame_wgrad_geometry(576 * 29, 2) == (261, 64)
    assert R.frame_wgrad_geometry(576 * 30, 4) == (256, 68) and R.frame_wgrad_geometry(576 * 30, 1) == (270, 64)
    assert R.frame_wgrad_geometry(1, 5) == (1, 4) and R.frame_wgrad_geometry(130, 5) == (2, 68) and R.frame_wgrad_geometry(130, 0) == (2, 68)
    for which, (Co, Ci, budget, _) in enumerate(R.FRAME_WG):                   # the largest chunk count fits every budget
        assert R.frame_wgrad_geometry(R.CHUNK * 576, which)[0] * Co * Ci <= budget
