"""The CPU references of the forward streaming launches (tests/stream_ops_ref.py) checked against themselves, without a GPU:
  1. ref64 equals the float64 torch modules of the operation (F.max_pool2d, F.interpolate(bilinear, align_corners=True) + cat,
     F.group_norm(., 1, .), F.layer_norm, F.mish, F.silu, F.gelu, F.conv2d) to 1e-12 of the scale S, per element; film_coef's
     A x + B equals film_apply's reference; the float32 scheduler step equals oracle/scheduler_ref.py bit for bit;
  2. every mutant of every op violates TAU * S on some element of some case of that op;
  3. ref32 is within its own bound, TAU is finite, and tests/golden/stream_ops_tau.json holds the values the references produce;
  4. expected_info restates conv_in_parts and combine_rows (csrc/elementwise.hip, csrc/kernels.h) on known values.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_ops_ref as R
import train_ops_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_ops_tau.json")
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
    # per element to 1e-12 of S; where S is zero (copies, padding) or tiny, to 1e-14 of the output's largest value: torch takes
    # the statistics from x itself, and x - mean at mean -300 costs it a few hundred float64 roundings
    floor = 1e-2 * float(np.abs(want).max()) if want.size else 0.0
    bad = ~(np.abs(ref - want) <= rel * np.maximum(np.maximum(scale, np.abs(want)), floor))
    assert not bad.any(), (name, int(bad.sum()), float(np.abs(ref - want).max()))


def _gn(x, g, n=None):
    """GroupNorm(1, cnorm) of the real lanes of x [B][HW][C] by torch in float64, zeros in the padded lanes: [B][HW][n]"""
    x = T64(x)[:, :, :n]
    if g is None:
        return x
    cn = min(g["cnorm"], x.shape[2])
    y = F.group_norm(x[:, :, :cn].permute(0, 2, 1), 1, T64(g["gamma"][:cn]), T64(g["beta"][:cn]), R.EPS).permute(0, 2, 1)
    out = torch.zeros_like(x)
    out[:, :, :cn] = y
    return out


def _img(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _rows(t):
    B, C = t.shape[:2]
    return t.permute(0, 2, 3, 1).reshape(B, -1, C)


def _t_rows(inp, B):
    t = np.asarray(inp["t"])
    return torch.from_numpy(np.repeat(t, B) if len(t) == 1 else t).long()


def _film(inp, v):
    B, C = inp["B"], inp["C"]
    if inp["temb"] is not None:
        v = v + T64(inp["temb"])[_t_rows(inp, B)][:, None, :]
    if inp["film"] is not None:
        f = T64(inp["film"])
        v = f[:, None, :C] * v + f[:, None, C:]
    return v


def _torch(op, inp):
    """{output name: float64 torch value} of the op's torch expression"""
    B = inp.get("B")
    if op == "conv_in":
        H0, D, Hp, Wp, lh, lw = (inp[k] for k in ("H0", "D", "Hp", "Wp", "lh", "lw"))
        x = F.pad(T64(inp["x"])[:, None], (lw, Wp - D - lw, lh, Hp - H0 - lh))
        w = T64(inp["w"]).T.reshape(64, 1, 3, 3)
        y = _rows(F.conv2d(x, w, padding=1))
        yp = y.reshape(B, inp["parts"], -1)
        return {"dst": y, "stats": torch.stack([yp.sum(2), (yp * yp).sum(2)], 2)}
    if op == "pool":
        H, W = inp["H"], inp["W"]
        return {"dst": _rows(F.max_pool2d(_img(_gn(inp["x"], inp["gn"]), B, H, W), 2))}
    if op == "upcat":
        Hin, Win = inp["Hin"], inp["Win"]
        up = F.interpolate(_img(_gn(inp["up"], inp["gn"]), B, Hin, Win), scale_factor=2, mode="bilinear", align_corners=True)
        parts = [_rows(up)] + ([_gn(inp["skip"], inp["gn_skip"])] if inp["Cs"] else [])
        return {"dst": torch.cat(parts, 2)}
    if op == "film_apply":
        y = _film(inp, _gn(inp["x"], inp["gn"]))
        out = {"dst": y}
        if inp["row_stats"]:
            out["row_stats"] = torch.stack([y.sum(2), (y * y).sum(2)], 2)
        return out
    if op == "layernorm":
        return {"y": F.layer_norm(T64(inp["x"]), (inp["C"],), T64(inp["g"]), T64(inp["b"]), R.EPS)}
    if op in ("mish_pad", "silu_pad"):
        f = F.mish if op == "mish_pad" else F.silu
        return {"dst": F.pad(f(T64(inp["cond"])), (0, inp["Kp"] - inp["cond_dim"]))}
    if op == "silu":
        return {"y": F.silu(T64(inp["x"]))}
    if op == "dc_finish":
        v = _gn(inp["x"], inp["gn"])
        return {"dst": F.gelu(v if inp["res"] is None else v + T64(inp["res"]))}
    if op == "simple_tail":
        Cr, Co, HW = inp["Cr"], inp["Co"], inp["HW"]
        y = F.gelu(_gn(inp["x"], inp["gn"], Cr)) + T64(inp["temb"])[_t_rows(inp, B)][:, None, :Cr]
        cemb = T64(inp["cemb"])[:, None, :32].expand(B, HW, 32)
        return {"dst": torch.cat([y, cemb, torch.zeros(B, HW, Co - Cr - 32, dtype=torch.float64)], 2)}
    if op == "splitk_combine":
        y = T64(inp["partial"]).sum(0)
        yb = y.reshape(B, inp["HW"] // R.combine_rows(inp["HW"], inp["N"]), -1)
        return {"dst": y, "stats": torch.stack([yb.sum(2), (yb * yb).sum(2)], 2)}
    return {}


@pytest.mark.parametrize("op,case", ALL, ids=IDS)
def test_ref64_is_the_torch_module_in_float64(op, case):
    inp, ref, scale, _ = case_data(op, case)
    for k, v in ref.items():
        assert np.isfinite(v).all() and np.isfinite(scale[k]).all() and (scale[k] >= 0).all(), (op, k)
    for name, want in _torch(op, inp).items():
        _close(f"{op}/{case[0]}/{name}", ref[name], want, scale[name])
    if op == "conv_in" and inp["adv"] >= -1:                                   # the bookkeeping: exact
        step = inp["adv"] if inp["adv"] >= 0 else inp["step0"] + 1
        assert ref["words"].tolist() == [step, int(inp["timesteps"][min(step, inp["n_steps"] - 1)])] and not scale["words"].any()
    if op == "film_coef":                                                      # y = A x + B is film_apply's y
        C = inp["C"]
        ab = ref["ab"]
        y = ab[:, None, :C] * inp["x"].astype(np.float64) + ab[:, None, C:]
        fa = dict(inp, row_stats=False)
        _close(f"{op}/{case[0]}/A x + B", R.ref64("film_apply", fa)["dst"], y, R.scale64("film_apply", fa)["dst"], rel=1e-11)


@pytest.mark.parametrize("op", R.OPS)
def test_where_the_scale_is_zero_the_references_agree_exactly(op):
    """equality is meant, and only there: padding, copies, the words, a MaxPool without GroupNorm, the restated scheduler step"""
    seen_zero = False
    for case in R.cases(op):
        inp, ref, scale, tau = case_data(op, case)
        r32 = R.ref32(op, inp)
        for k in ref:
            z = scale[k] == 0
            seen_zero |= bool(z.any())
            assert np.array_equal(r32[k][z], ref[k][z]), (op, case[0], k)
    if op in ("conv_in", "pool", "upcat", "mish_pad", "silu_pad", "simple_tail", "out_step"):
        assert seen_zero, op                                                   # the ops with an exact part have a case that shows it


def _oracle_schedule(kind, T_, n):
    from oracle.scheduler_ref import LinearBetaSchedule
    s = LinearBetaSchedule(T_)
    s.set_timesteps(n)
    return s


@pytest.mark.parametrize("kind", (0, 1))
def test_scheduler_step_is_the_oracles_bit_for_bit(kind):
    from oracle.scheduler_ref import ddim_step, ddpm_step
    T_, n = 20, 5
    coef, ts = R.coef_table(kind, T_, n)
    s = _oracle_schedule(kind, T_, n)
    assert ts == s.timesteps.tolist()
    rng = np.random.default_rng(11 + kind)
    x, eps, z = (rng.standard_normal((3, 16, 3)).astype(np.float32) for _ in range(3))
    for i, t in enumerate(ts):
        tx, te, tz = (torch.from_numpy(v) for v in (x, eps, z))
        want = ddpm_step(s, te, t, tx, tz) if kind == 0 else ddim_step(s, te, t, tx)
        mine = R.step_f32(kind, coef[i], x, eps, z)
        assert mine.dtype == np.float32 and mine.tobytes() == want.numpy().tobytes(), (kind, i, t)
    assert coef[-1][5] == 0 and (kind == 1 or (coef[:-1, 5] > 0).all())       # no noise at t == 0


def test_out_step_is_the_restated_step_with_inpainting_and_history():
    for case in R.cases("out_step"):
        inp, ref, scale, _ = case_data("out_step", case)
        if inp["mode"] == 0 or inp["flavour"] == "nonfinite":
            continue
        i, h = inp["step"], inp["inp_h"]
        eps = inp["eps"] if inp["mode"] == 2 else None
        if eps is not None and (inp["noise"] is not None or inp["kind"] == 1 or inp["coef"][i][5] == 0):
            z = None if inp["noise"] is None else inp["noise"][i]
            want = R.step_f32(inp["kind"], inp["coef"][i], inp["x"], eps, z).astype(np.float64)
            if h:
                want[:, :h] = inp["inpaint"]
            assert np.array_equal(ref["x"], want) and not scale["x"].any(), case[0]
        if inp["history"] is not None:
            assert np.array_equal(ref["history"][i + 1], ref["x"])
            keep = np.arange(inp["n_steps"] + 1) != i + 1
            assert np.array_equal(ref["history"][keep], inp["history"].astype(np.float64)[keep])
        if h:
            assert np.array_equal(ref["x"][:, :h], np.broadcast_to(inp["inpaint"].astype(np.float64), ref["x"][:, :h].shape))
    inp, ref, _, _ = case_data("out_step", [c for c in R.cases("out_step") if c[0] == "nonfinite_features_full_step"][0])
    assert ref["flag"][0] == 1 and sorted(set(ref["nonfinite"].ravel().tolist()) - {0.0}) in ([1.0, 3.0], [2.0, 3.0])
    assert (ref["nonfinite"] > 0).sum() == 2                                   # nothing else is disturbed


def test_philox_uniforms_are_the_oracles_stream():
    from oracle.philox_ref import step_noise
    inp = R.make_inputs("out_step", [c for c in R.cases("out_step") if c[0] == "philox_mid_direct"][0])
    B, HD = inp["B"], inp["H0"] * inp["D"]
    z = R._philox_normal(inp, np.float32, False)
    want = step_noise(inp["seed"], inp["step"], inp["first"], B, HD)
    assert inp["seed"] >> 32 and inp["first"] > 0
    np.testing.assert_allclose(z, want, rtol=0, atol=2e-6)


@pytest.mark.parametrize("op", R.OPS)
def test_every_mutant_violates_the_bound(op):
    missed = set(R.MUTANTS[op])
    assert len(missed) >= 2
    for case in R.cases(op):
        inp, ref, scale, tau = case_data(op, case)
        for m in sorted(missed):
            if R.worst_ratio(R.ref64(op, inp, mutant=m), ref, scale, tau) > 1.0:
                missed.discard(m)
        if not missed:
            break
    assert not missed, (op, sorted(missed))


@pytest.mark.parametrize("op", R.OPS)
def test_ref32_within_its_own_bound(op):
    for case in R.cases(op):
        inp, ref, scale, tau = case_data(op, case)
        assert np.isfinite(tau) and tau >= 0
        assert R.worst_ratio(R.ref32(op, inp), ref, scale, tau) <= (1.0 if op in R.FLOOR_U else 0.2500001), (op, case[0])
        assert tau < 1e-3, (op, case[0], tau)                                   # a bound that would pass anything is no bound


def test_every_consumer_sees_every_statistics_path():
    """per GroupNorm consumer: no statistics, the serial path, one slot per lane, the i += 64 stride, tiles that straddle samples,
    cnorm < C, a variance that clamps; unused slots are NaN"""
    for op in R.GN_CONSUMERS:
        seen = set()
        for case in R.cases(op):
            inp = case_data(op, case)[0]
            for g in (inp["gn"], inp.get("gn_skip")):
                if g is None:
                    seen.add("none")
                    continue
                reads = R.gn_reads(g["stats"].shape[0], g["HW"], g["m_tile"], g["n_tiles"])
                for b, n in enumerate(reads):
                    seen.add("serial" if n <= 8 else "lanes" if n <= 64 else "stride")
                    assert np.isfinite(g["stats"][b, :n]).all() and np.isnan(g["stats"][b, n:]).all() and g["slots"] > n
                if g["HW"] % g["m_tile"] and len(reads) >= 3:
                    seen.add("straddle")
                if g["cnorm"] < g["C"]:
                    seen.add("cnorm")
                m = g["stats"][0, :reads[0]].sum(0) / (g["cnorm"] * g["HW"])
                if m[1] - m[0] ** 2 < 0:
                    seen.add("clamp")
        assert seen == {"none", "serial", "lanes", "stride", "straddle", "cnorm", "clamp"}, (op, seen)


def _table():
    return {f"{op}/{case[0]}": case_data(op, case)[3] / R.U for op, case in ALL}


def test_the_golden_tau_table_is_current():
    """TAU of every case in units of u, as the references produce it here on the CPU (never from a device)"""
    want = json.load(open(GOLDEN))
    got = _table()
    assert set(got) == set(want)
    for k, v in got.items():
        assert abs(v - want[k]) <= 1e-6 * max(1.0, abs(want[k])), (k, v, want[k])


def test_the_training_tau_rule_is_unchanged():
    """tau() was generalised for this family; the training ops go through the same code with their own references"""
    case = T.cases("ln_fwd")[0]
    inp = T.make_inputs("ln_fwd", case)
    assert T.tau("ln_fwd", inp) == T.tau("ln_fwd", inp, refs=(T.ref64, T.scale64, T.ref32, T.FLOOR_U))


def test_expected_info_restates_the_launch_geometry():
    assert [R.combine_rows(hw, n) for hw, n in ((4, 64), (16, 256), (64, 512), (9, 512), (25, 512), (64, 64))] == [4, 8, 4, 9, 25, 32]
    assert [R.conv_in_parts(hw, b) for hw, b in ((64, 1), (512, 1023), (512, 1024), (96, 1))] == [4, 4, 1, 1]
    assert R.stats_slots(512, 128, 1) == 5 and R.stats_slots(512, 512, 1) == 2 and R.stats_slots(25, 25, 1) == 2 and R.stats_slots(9, 1, 1) == 9
    for op in ("conv_in", "splitk_combine"):
        for case in R.cases(op):
            inp = case_data(op, case)[0]
            first, slots = R.expected_info(op, inp)
            P = R.launch_plan(op, inp)
            assert P["stats_out"] == inp["B"] * slots * 2 and P["outs"]["stats"][2] == slots * 2
            assert first == (case[1]["parts"] if op == "conv_in" else R.combine_rows(inp["HW"], inp["N"]))
    assert {c[1]["parts"] for c in R.cases("conv_in")} == {1, 4}


if __name__ == "__main__":                                                     # regenerate the table (CPU only; repository root on PYTHONPATH)
    json.dump(_table(), open(GOLDEN, "w"), indent=0, sort_keys=True)
