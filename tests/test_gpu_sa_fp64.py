"""The SelfAttention routes on weights whose softmax is peaked, against the oracle in float64 (whole model) and against each
other, and the training gradients through peaked attention against float64 autograd.

random_state_dict's in_proj rows keep every logit below 1.7, so the softmax of all six blocks is close to uniform (max p L <=
3.5) and neither the running-max rescale of the key-block loops, nor exp at large negative arguments, nor P x 1024 split with
one p ~ 1, nor a dropped `lo` term of q or k is visible in eps.  `sharpen` scales the q and k rows of every in_proj weight and
bias by g (logits x g^2): 'moderate' g = 4 (logit range per query 13-40, median max-p 0.3-0.8), 'onehot' g = 6 (27-90,
0.66-0.98), 'onehot+widened' g = 6 on tests/test_gpu_parity._widened (FiLM x 3, GroupNorm gains negative / zero).

Block by block (test_blocks_against_float64_under_sa_bound): a debug handle's input tap of each block goes through
sa_ref.sa_block_ref in float64 and the output tap must lie within sa_ref.sa_bound per element.  Worst measured
err / (A + SV / 1024), x 1e-9, per route (columns plain / moderate / onehot / onehot+widened), first run on the MI355X:
    default, SPDM_SA_NO_WLDS   3.4   4.8    8.9   12.3
    SPDM_SA_HEAD               3.3   3.9    8.8   10.9
    SPDM_NO_SA_FUSED           3.2   5.6    7.0   11.7
      + SPDM_ATTN_VALU         6.0   5.8    7.9   12.0
    SPDM_NO_SA_TAIL            3.5   4.2    8.4   11.9
    exact_fp32                 3.6   4.4   12.5   10.1
Worst 1.25e-8 -> TAU = 3.5e-8 (2.8 x), TAU_S = TAU / 1024 (sa_ref.py says why the S V term is small); per block the worst is
sa6 (6.0 / 5.8 / 12.5 / 12.3) and the best sa3 (0.7 / 1.0 / 1.3 / 2.5).  The routes below that a debug handle cannot reach
(FiLM folded or evaluated in the consumers, cropped sa6 with and without outc) are held here on eps of the whole model, and per
element, one launch at a time, by tests/test_gpu_sa_ops_fp64.py.

Every case prints the kernels each block takes (`block_routes` / `film_routes`, restating Ctx::choose_routes' rules in
spdm_api.hip, and asserted equal to the planner's own choice, SpdmEngine.plan_routes: `assert_plan`) and
  ROUTE <flavour> H D B <route>: max |eps - eps64| / scale, max |eps - eps_default| / scale
Tolerances (relative to max(1, max |eps64|)): TOL64 against float64, TOL_ROUTES between routes of the split path.  They were set
from the first measured run on the MI355X (seeded data, deterministic kernels) with at most 4 x margin over the worst figure,
and may not exceed the project's 1e-4.  Worst measured per route (x 1e-6; columns moderate / onehot / onehot+widened):
    route                 moderate        onehot          onehot+widened      (error against float64 / against the default route)
    default               1.15 / -        2.48 / -        0.95 / -
    debug handle          0.96 / 0.48     2.42 / 0.81     1.04 / 0.83
    SPDM_SA_HEAD          0.90 / 0.44     2.46 / 0.81     1.00 / 0.72
    SPDM_NO_SA_FUSED      0.95 / 0.48     2.31 / 0.77     0.96 / 0.52
      + SPDM_ATTN_VALU    0.90 / 0.54     3.01 / 0.92     0.96 / 0.63
    SPDM_NO_SA_TAIL       0.93 / 0.51     2.58 / 0.92     1.08 / 0.60
    SPDM_SA_NO_WLDS       0.90 / 0        2.48 / 0        0.95 / 0            (bit-identical to the default route)
    SPDM_FILM_LOCAL       1.15 / 0        2.48 / 0        0.95 / 0            (bit-identical to film_coef)
    SPDM_NO_FILM_FOLD     1.33 / 0.74     2.54 / 1.51     1.03 / 0.77
    SPDM_NO_SA_CROP       1.14 / 0.25     2.48 / 0.25     0.97 / 0.31         (moderate, and the 0.25s: the B = 300 test; else the sweep)
    SPDM_NO_SA_OUTC       1.14 / 0.25     2.48 / 0.25     0.97 / 0.31
    exact_fp32            1.67 / (1.94)   2.81 / (2.92)   2.12 / (2.21)       (agreement with the split path is not asserted)
    B = 2048, plan's rule      -          2.24 / 2.53          -              (sa_head for sa1 against SPDM_NO_SA_HEAD)
The worst case against float64 is 3.01e-6 ('onehot', H 32, D 3, B 37), the worst between split routes 2.53e-6: TOL64 = TOL_ROUTES
= 1e-5 (3.3 x and 3.9 x).  For scale: on the same inputs (H 32, D 3, B 37) the fp32 CPU oracle is 0.96e-6 / 2.18e-6 / 1.10e-6
from float64 (0.84e-6 at g = 1, same inputs), so every route is as close to float64 as fp32 arithmetic on the CPU is.
Training (SpdmEngine(train_attention=True)): bound unchanged from tests/test_gpu_train_grad_attn.py (relative L2 per tensor
<= 1e-4, loss 1e-6); in addition the in_proj gradients of sa3 and sa6 per element, |g - g64| <= 1e-4 max |g64|.
Measured: worst tensor 7.7e-6 / 9.2e-6 ('moderate', B 2 / B 5) and 2.2e-5 / 1.5e-5 ('onehot'); loss 2e-7 or better; per
element, sa3 in_proj 5.7e-6 .. 1.9e-5 and sa6 in_proj 4e-7 .. 3.7e-6 of max |g64|.  All inside the unchanged bound.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from oracle.unet_film_ref import unet_film_forward
from sa_ref import BLOCKS, COND, flavour_weights, inputs, sa_block_ref, sa_bound
from test_gpu_train_grad_attn import BOUND, _assert_within, _check, _oracle_loss_grad, _print_classes

pytestmark = pytest.mark.gpu

CD = COND[0] * COND[1]
TOL64 = 1e-5
TOL_ROUTES = 1e-5
_REF = {}


def oracle64(flavour, H, D, B, idx=None):
    """eps of the float64 oracle for the samples idx (all when None): one evaluation per (flavour, geometry)."""
    key = (flavour, H, D, B, None if idx is None else tuple(idx))
    if key not in _REF:
        sd = {k: v.double() for k, v in flavour_weights(flavour).items()}
        x, y, t = inputs(H, D, B)
        sel = slice(None) if idx is None else list(idx)
        _REF[key] = unet_film_forward(sd, x[sel].double(), t[sel], y[sel].double())
    return _REF[key]


@contextlib.contextmanager
def engine(H, D, B, sd, env=None, **kw):
    """A handle created under the route's environment (read once, at creation)."""
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = SpdmEngine(H, D, CD, max_batch=B, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    try:
        eng.load_state_dict(sd)
        yield eng
    finally:
        eng.close()


# ---- which kernels a block takes (Ctx::choose_routes, spdm_api.hip; sa_*_supported in sa_fused.hip / sa_tail.hip) -----
def block_shapes(H, D):
    Hp, Wp = -(-H // 8) * 8, -(-D // 8) * 8
    hw = lambda lvl: (Hp >> lvl) * (Wp >> lvl)
    return {"sa1": (128, hw(1)), "sa2": (256, hw(2)), "sa3": (256, hw(3)), "sa4": (128, hw(2)), "sa5": (64, hw(1)),
            "sa6": (64, hw(0))}


def sa_head_supported(C, L):
    return C in (128, 256) and (8192 // C) % L == 0


def sa_crop_supported(L, H, D):
    return H * D < L <= 256 and H * D <= 32 * min(4, (L + 31) // 32)


def block_routes(H, D, B, env, exact=False, debug=False):
    out = {}
    for name, (C, L) in block_shapes(H, D).items():
        if exact:
            core = "attn_valu" if L < 32 or "SPDM_ATTN_VALU" in env else "attn_mfma"
            out[name] = f"gemm_fp32+{core}+gemm_fp32"
        elif C == 64 and L <= 512 and "SPDM_NO_SA_FUSED" not in env:
            r = "sa_fused64" + ("_2wg" if L > 256 else "") + ("_nowlds" if "SPDM_SA_NO_WLDS" in env else "")
            if name == "sa6" and not debug and "SPDM_NO_SA_CROP" not in env and sa_crop_supported(L, H, D):
                r = "sa_crop64" + ("" if "SPDM_NO_SA_OUTC" in env else "+outc")
            out[name] = r
        else:
            tail = C in (128, 256) and "SPDM_NO_SA_TAIL" not in env
            tiles = -(-B * L // (8192 // C))
            core = "attn_valu" if L < 32 or "SPDM_ATTN_VALU" in env else "attn_mfma"
            if tail and sa_head_supported(C, L) and "SPDM_NO_SA_HEAD" not in env and ("SPDM_SA_HEAD" in env or tiles >= 2048):
                out[name] = "sa_head+sa_tail"
            else:
                out[name] = ("sa_qkv" if tail else "gemm") + "+" + core + "+" + ("sa_tail" if tail else "gemm x3")
    return out


def sa_tail_film_local(C, L):
    """sa_tail.hip: one [A | B] row of 2 C floats per sample a tile of 8192 / C rows can touch, within 24 KB of LDS."""
    return C in (128, 256) and L >= 1 and ((8192 // C + L - 2) // L + 1) * 2 * C * 4 <= 24 * 1024


FILM = ("film_apply", "film_coef", "film_local")


def film_routes(H, D, B, env, debug=False, exact=False):
    """The FiLM tail in front of each block: applied by film_apply, folded into the block's loads as film_coef's coefficients
    (the kernels that read the block input themselves: sa_fused64 up to 256 tokens, sa_qkv / sa_tail), or evaluated inside those
    kernels (batch <= 4, or SPDM_FILM_LOCAL, where their LDS holds the coefficient rows)."""
    out = {}
    for name, (C, L) in block_shapes(H, D).items():
        fused = not exact and C == 64 and L <= 512 and "SPDM_NO_SA_FUSED" not in env
        tail = not exact and C in (128, 256) and "SPDM_NO_SA_TAIL" not in env
        fold = not (debug or exact or "SPDM_NO_FILM_FOLD" in env) and (L <= 256 if fused else tail)
        local = fold and (B <= 4 or "SPDM_FILM_LOCAL" in env) and (fused or sa_tail_film_local(C, L))
        out[name] = FILM[2 if local else 1 if fold else 0]
    return out


def route_key(route):
    """A block_routes string as the planner reports the block (SpdmEngine.plan_routes): (fused, crop, outc, in, tail); the
    attention core's kernel and sa_fused64's variants are the launchers' choice, not the plan's."""
    if route.startswith("sa_crop64"):
        return (1, 1, int(route.endswith("+outc")), 0, 0)
    if route.startswith("sa_fused64"):
        return (1, 0, 0, 0, 0)
    parts = route.split("+")
    return (0, 0, 0, {"sa_head": 2, "sa_qkv": 1}.get(parts[0], 0), int(parts[-1] == "sa_tail"))


def assert_plan(eng, H, D, B, env, exact=False, debug=False, attention=True):
    """The planner's own choice for this handle equals the restatements above; returns them for printing."""
    plan = eng.plan_routes(B)
    blocks, films = block_routes(H, D, B, env, exact, debug), film_routes(H, D, B, env, debug, exact)
    if not attention:       # no SelfAttention blocks: film_apply finishes every tail, nothing else is launched
        blocks, films = {name: "none" for name in blocks}, {name: "film_apply" for name in films}
    for i, name in enumerate(blocks):
        want = (route_key(blocks[name]), films[name])
        got = (tuple(plan["sa"][i][k] for k in ("fused", "crop", "outc", "in", "tail")), FILM[plan["film"][i]])
        assert got == want, (name, got, want, H, D, B, env)
    return blocks, films


# (name, environment, engine keywords)
ROUTES = [
    ("default", {}, {}),
    ("debug", {}, dict(debug=True)),
    ("sa_head", {"SPDM_SA_HEAD": "1"}, {}),
    ("no_sa_fused", {"SPDM_NO_SA_FUSED": "1"}, {}),
    ("no_sa_fused+valu", {"SPDM_NO_SA_FUSED": "1", "SPDM_ATTN_VALU": "1"}, {}),
    ("no_sa_tail", {"SPDM_NO_SA_TAIL": "1"}, {}),
    ("sa_no_wlds", {"SPDM_SA_NO_WLDS": "1"}, {}),
    ("film_local", {"SPDM_FILM_LOCAL": "1"}, {}),
    ("no_film_fold", {"SPDM_NO_FILM_FOLD": "1"}, {}),
    ("no_sa_crop", {"SPDM_NO_SA_CROP": "1"}, {}),
    ("no_sa_outc", {"SPDM_NO_SA_OUTC": "1"}, {}),
    ("exact_fp32", {}, dict(exact_fp32=True)),
]
# (H, D, B): L = 512 at (64, 6) is the two-workgroup form of sa_fused64; (24, 4) and (40, 2) have token counts that are not
# powers of two (192 / 48 / 12 / 3 and 320 / 80 / 20 / 5: masked key tails)
GEOMS = [(32, 3, 1), (32, 3, 3), (32, 3, 37), (16, 3, 9), (64, 6, 5), (24, 4, 5), (40, 2, 2)]


def _applies(route, H, D, B):
    shapes = block_shapes(H, D)
    if route == "sa_head":        # sa_head_supported: the 8192 / C row tile must hold whole samples -- no block of (24, 4), (40, 2)
        return any(sa_head_supported(C, L) for C, L in shapes.values())
    if route in ("no_sa_crop", "no_sa_outc"):       # sa_crop_supported: H D < L <= 256 -- not (40, 2) (L = 320), (64, 6) (512)
        return sa_crop_supported(shapes["sa6"][1], H, D)
    if route == "film_local":     # B <= 4 evaluates the coefficients in the consumers by default: the switch changes nothing
        return B > 4
    return True


# routes whose kernels differ from the default's in arithmetic: eps must differ in some bit, or the switch is dead
DIFFERENT_KERNELS = ("debug", "sa_head", "no_sa_fused", "no_sa_fused+valu", "no_sa_tail", "no_film_fold", "no_sa_crop",
                     "no_sa_outc", "exact_fp32")
CASES = [(f, g) for f in ("moderate", "onehot", "onehot+widened") for g in GEOMS]


def _run(eng, H, D, B):
    x, y, t = inputs(H, D, B)
    got = eng.unet_forward(x.cuda(), t, y.cuda()).cpu().double()
    assert not eng.nonfinite()
    return got


@pytest.mark.parametrize("flavour,geom", CASES, ids=[f"{f}-H{g[0]}D{g[1]}B{g[2]}" for f, g in CASES])
def test_routes_against_float64_oracle(flavour, geom):
    H, D, B = geom
    sd = flavour_weights(flavour)
    want = oracle64(flavour, H, D, B)
    scale = max(1.0, float(want.abs().max()))
    base = None
    for name, env, kw in ROUTES:
        if not _applies(name, H, D, B):
            continue
        with engine(H, D, B, sd, env, **kw) as eng:
            got = _run(eng, H, D, B)
            if not kw.get("exact_fp32"):
                assert eng.split_precision and eng.demoted_tensors == 0, name     # the split path really ran
            blocks, films = assert_plan(eng, H, D, B, env, kw.get("exact_fp32", False), kw.get("debug", False))
        if base is None:
            base = got
        e64 = float((got - want).abs().max()) / scale
        ert = float((got - base).abs().max()) / scale
        print(f"\nROUTE {flavour} {H} {D} {B} {name}: {e64:.3e} {ert:.3e} scale {scale:.2f} {films} {blocks}")
        assert e64 <= TOL64, (flavour, geom, name, e64)
        if not kw.get("exact_fp32"):
            assert ert <= TOL_ROUTES, (flavour, geom, name, ert)
        if name in DIFFERENT_KERNELS:
            assert ert > 0.0, (flavour, geom, name, "bit-identical to the default route: the switch did not take effect")


@pytest.mark.parametrize("flavour", ["moderate", "onehot"])
def test_film_coef_and_cropped_sa6_at_batch_300(flavour):
    """B = 300: film_coef (B > 4) and the query-cropped sa6 with and without outc in its epilogue; the oracle on a subset."""
    H, D, B = 32, 3, 300
    idx = [0, 1, 63, 64, 127, 128, 255, 256, B - 1]
    sd = flavour_weights(flavour)
    want = oracle64(flavour, H, D, B, idx)
    scale = max(1.0, float(want.abs().max()))
    base = None
    for name, env, kw in ROUTES:
        if name not in ("default", "no_sa_crop", "no_sa_outc", "no_film_fold", "film_local"):
            continue
        with engine(H, D, B, sd, env, **kw) as eng:
            got = _run(eng, H, D, B)
            assert eng.demoted_tensors == 0
            blocks, films = assert_plan(eng, H, D, B, env)
        base = got if base is None else base
        e64 = float((got[idx] - want).abs().max()) / scale
        ert = float((got - base).abs().max()) / scale
        print(f"\nROUTE {flavour} {H} {D} {B} {name}: {e64:.3e} {ert:.3e} scale {scale:.2f} {films} {blocks}")
        assert e64 <= TOL64, (flavour, name, e64)
        assert ert <= TOL_ROUTES, (flavour, name, ert)
        if name in DIFFERENT_KERNELS:
            assert ert > 0.0, (flavour, name, "bit-identical to the default route")


def test_sa_head_chosen_by_the_plan_at_batch_2048():
    """The plan's own rule takes sa_head_kernel from 2048 row tiles of 8192 / C rows: at H = 32, D = 3, B = 2048 that is sa1
    (2048 x 64 rows / 64) and no other block; SPDM_NO_SA_HEAD is the three-launch path.  Oracle on: first, last, both sides of
    every 64-sample boundary among 8 seeded ones."""
    H, D, B = 32, 3, 2048
    tiles = {n: -(-B * L // (8192 // C)) for n, (C, L) in block_shapes(H, D).items() if C != 64}
    assert tiles == {"sa1": 2048, "sa2": 1024, "sa3": 256, "sa4": 512}
    routes = block_routes(H, D, B, {})
    assert [n for n, r in routes.items() if r.startswith("sa_head")] == ["sa1"]
    bnd = np.random.default_rng(3).choice(np.arange(1, B // 64), 8, replace=False) * 64
    idx = sorted({0, B - 1} | {int(b) - 1 for b in bnd} | {int(b) for b in bnd})
    flavour = "onehot"
    sd = flavour_weights(flavour)
    want = oracle64(flavour, H, D, B, idx)
    scale = max(1.0, float(want.abs().max()))
    with engine(H, D, B, sd) as eng:
        got = _run(eng, H, D, B)
        assert eng.demoted_tensors == 0
        assert_plan(eng, H, D, B, {})
    with engine(H, D, B, sd, {"SPDM_NO_SA_HEAD": "1"}) as eng:
        three = _run(eng, H, D, B)
        assert_plan(eng, H, D, B, {"SPDM_NO_SA_HEAD": "1"})
    e64 = float((got[idx] - want).abs().max()) / scale
    ert = float((got - three).abs().max()) / scale
    print(f"\nROUTE {flavour} {H} {D} {B} plan: {e64:.3e} {ert:.3e} scale {scale:.2f} film_coef {routes}")
    assert ert > 0.0                    # the two paths are different kernels: identical bits would mean the rule did not switch
    assert e64 <= TOL64, e64
    assert ert <= TOL_ROUTES, ert


# ---- the planner's choice against the restatements, on both sides of every threshold the rules have ------------------------
# (id, H, D, B, environment, engine keywords).  H = 32, D = 3: coefficients in the consumers up to B = 4; pool 1 by its producer
# from 256, pool 2 from 257, pool 3 from 1025 (tests/test_gpu_pooled_epilogue.py); sa_head for sa1 from 2048.  H = 16: pool 1
# refused below conv_reg64's smallest map.  H = 64, D = 6: the two-workgroup sa_fused64 (no FiLM fold, no crop).
PLAN_CASES = ([(f"B{B}", 32, 3, B, {}, {}) for B in (4, 5, 255, 256, 257, 1024, 1025, 2047, 2048)] +
              [("H16", 16, 3, 2049, {}, {}), ("H64", 64, 6, 5, {}, {}),
               ("debug", 32, 3, 1025, {}, dict(debug=True)), ("no_attention", 32, 3, 1025, {}, dict(attention=False))] +
              [(name, 32, 3, 1025, env, kw) for name, env, kw in ROUTES if name not in ("default", "debug")] +
              [("no_reg64", 32, 3, 1025, {"SPDM_NO_REG64": "1"}, {}), ("no_fused_src", 32, 3, 1025, {"SPDM_NO_FUSED_SRC": "1"}, {}),
               ("no_fused_src-B5", 32, 3, 5, {"SPDM_NO_FUSED_SRC": "1"}, {})])


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_planner_choice_matches_the_restatements(case):
    """spdm_debug_plan_routes (host arithmetic) against block_routes / film_routes here and expected_pools of
    tests/test_gpu_pooled_epilogue.py.  The restatements have no opinion on read-through versus two-source for the up blocks:
    there, one unet_forward must make as many launches that read the upsample through conv_wide's loader
    (spdm_debug_fused_upsample_launches counts those, not the small-grid kernel's) as the planner reports up blocks read through
    whose first convolution spdm_debug_geometry does not put on the small-grid kernel."""
    from state_policy_diffusionmodel_amd import _lib
    from state_policy_diffusionmodel_amd.weights import random_state_dict
    from test_gpu_pooled_epilogue import _geometry, expected_pools
    _, H, D, B, env, kw = case
    exact, debug, attention = kw.get("exact_fp32", False), kw.get("debug", False), kw.get("attention", True)
    count = _lib.load().spdm_debug_fused_upsample_launches
    with engine(H, D, B, random_state_dict(CD, seed=5, attention=attention), env, **kw) as eng:
        plan = eng.plan_routes(B)
        blocks, films = assert_plan(eng, H, D, B, env, exact, debug, attention)
        print(f"\nPLAN {case[0]} {H} {D} {B}: {plan['pool']} {plan['up']} {films} {blocks}")
        assert all(r in (0, 1, 2) for r in plan["pool"] + plan["up"])           # exactly one route per resampling op
        want = 0 if exact or debug else expected_pools(H, B, attention=attention and "SPDM_NO_SA_TAIL" not in env,
                                                        no_reg64="SPDM_NO_REG64" in env, no_fused_src="SPDM_NO_FUSED_SRC" in env)
        assert sum(1 << i for i, r in enumerate(plan["pool"]) if r == 2) == want, (plan["pool"], want)
        if exact or debug or "SPDM_NO_FUSED_SRC" in env:       # nothing is read through or taken from two sources
            assert 1 not in plan["pool"] + plan["up"] and 2 not in plan["up"], plan
        c0 = int(count())
        _run(eng, H, D, B)
        through_wide = int(count()) - c0
    Hp, Wp = -(-H // 8) * 8, -(-D // 8) * 8
    wide = 0
    for i, (C, lvl) in enumerate(((512, 2), (256, 1), (128, 0))):               # the first convolution of up block i + 1: C -> C
        hw, w = (Hp >> lvl) * (Wp >> lvl), Wp >> lvl
        if plan["up"][i] == 1 and not _geometry(B * hw, C, C, hw, w, 9)["skinny"]:
            wide += 1
    assert through_wide == wide, (plan["up"], through_wide, wide)


# ---- block by block: device input tap -> float64 block -> device output tap ---------------------------------------------------
# the routes a debug handle reaches (FiLM is applied, sa6 runs on all tokens)
DEBUG_ROUTES = [r for r in ROUTES if r[0] in ("default", "sa_head", "no_sa_fused", "no_sa_fused+valu", "no_sa_tail",
                                               "sa_no_wlds", "exact_fp32")]
BLOCK_CASES = [(f, g) for f in ("plain", "moderate", "onehot", "onehot+widened") for g in GEOMS]


def block_taps(flavour, geom, env, kw):
    """One unet_forward on a debug handle: {block: (input tap, output tap)} as the device holds them."""
    H, D, B = geom
    with engine(H, D, B, flavour_weights(flavour), env, debug=True, **kw) as eng:
        _run(eng, H, D, B)
        if not kw.get("exact_fp32"):
            assert eng.split_precision and eng.demoted_tensors == 0
        assert_plan(eng, H, D, B, env, kw.get("exact_fp32", False), debug=True)      # (the routes the caller prints)
        return {b: (eng.debug_tensor(i).cpu(), eng.debug_tensor(o).cpu()) for b, (i, o) in BLOCKS.items()}


@pytest.mark.parametrize("flavour,geom", BLOCK_CASES, ids=[f"{f}-H{g[0]}D{g[1]}B{g[2]}" for f, g in BLOCK_CASES])
def test_blocks_against_float64_under_sa_bound(flavour, geom):
    H, D, B = geom
    sd = flavour_weights(flavour)
    worst = {}
    for name, env, kw in DEBUG_ROUTES:
        if not _applies(name, H, D, B):
            continue
        routes = block_routes(H, D, B, env, kw.get("exact_fp32", False), True)
        for blk, (xin, out) in block_taps(flavour, geom, env, kw).items():
            ref = sa_block_ref(sd, blk, xin)
            err = (out.double() - ref["out"]).abs()
            ratio = float((err / sa_bound(ref)).max())
            print(f"\nBLOCK {flavour} {H} {D} {B} {name} {blk} {routes[blk]}: ratio {ratio:.3f} err/A {float((err / ref['A']).max()):.3e} "
                  f"max err {float(err.max()):.3e}")
            if not ratio <= 1.0:
                worst[(name, blk)] = ratio
    assert not worst, worst


# ---- training ---------------------------------------------------------------------------------------------------------------
TRAIN_CD = 14
TRAIN_CASES = [(f, c) for f in ("moderate", "onehot") for c in ((2, 16, 3), (5, 32, 3))]


@pytest.mark.parametrize("flavour,case", TRAIN_CASES, ids=[f"{f}-B{c[0]}H{c[1]}D{c[2]}" for f, c in TRAIN_CASES])
def test_training_gradients_on_peaked_attention(flavour, case):
    from test_gpu_train_grad_attn import _data, _engine
    B, H, D = case
    sd = flavour_weights(flavour, TRAIN_CD, 11)
    x, t, cond, noise = _data(B, H, D, 5, "per_sample")
    loss64, eps64, g64, gc64 = _oracle_loss_grad(sd, x, t, cond, noise)
    eng = _engine(H, D, B, False, sd)
    try:
        loss, eps, grads, gcond = eng.loss_and_grad(x.cuda(), t, cond.cuda(), noise.cuda())
        torch.cuda.synchronize()
        grads = {k: v.detach().double().cpu() for k, v in grads.items()}
        gcond = gcond.double().cpu()
    finally:
        eng.close()
    print(f"\nTRAIN {flavour} {case}: loss rel {abs(float(loss) - float(loss64)) / float(loss64):.2e}")
    worst = {}
    assert set(grads) == set(g64)
    for name, want in g64.items():
        _check(grads[name], want, name, worst)
    _check(gcond.reshape(gc64.shape), gc64, "grad_cond", worst)
    _print_classes(f"{flavour} {case}", worst)
    elem = {}
    for blk in ("sa3", "sa6"):
        for leaf in ("in_proj_weight", "in_proj_bias"):
            n = f"{blk}.attention.{leaf}"
            elem[n] = float((grads[n] - g64[n]).abs().max() / g64[n].abs().max())
    print(f"\nTRAIN {flavour} {case}: worst tensor {max(worst.values()):.2e}; per element " +
          ", ".join(f"{k} {v:.2e}" for k, v in elem.items()))
    assert abs(float(loss) - float(loss64)) <= 1e-6 * float(loss64), (float(loss), float(loss64))
    _assert_within(worst)
    bad = {k: v for k, v in elem.items() if not v <= BOUND}
    assert not bad, bad
