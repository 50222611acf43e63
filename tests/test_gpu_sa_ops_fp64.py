"""Every forward SelfAttention kernel (csrc/sa_fused.hip, sa_tail.hip, attention.hip), one launch at a time (spdm_op_sa), against
the float64 references of tests/sa_ops_ref.py on data the test controls.

Whole-block launches (FUSED64, its cropped form with and without outc, and the chains QKV -> CORE -> TAIL and HEAD -> TAIL) meet
sa_ref.sa_bound with TAU and TAU_S unchanged, per element, on the ab-affine or FiLM'd input.  The partial launches QKV, HEAD,
TAIL and CORE alone meet |got - ref64| <= TAU_op S_op (+ the split format's subnormal floors), TAU_op from the two CPU
restatements alone (tests/golden/sa_ops_tau.json).  Data is admitted only if a plain float32 CPU evaluation of the same op is
within 0.5 of the bound on every element (tests/test_sa_ops_reference.py), so a failure here is a kernel's, not the data's.
Every output buffer is filled with NaN first: an element the launch should not write (the tokens outside a crop) must still be
NaN afterwards, one it should write fails if it is not.  Every case runs twice and must give equal bits, and asserts its route
from info[].  Identities held bit for bit: wlds against no_wlds, FilmSpec against ab produced by the FILM_COEF stream op.
Where B is large a fixed subset of samples is compared (sa_ops_ref.subset).

Measured worst ratio of error to bound per op: DESIGN.md 8.20.
"""
import ctypes

import numpy as np
import pytest
import torch

import sa_ops_ref as R

pytestmark = pytest.mark.gpu

W_NAMES = ("attention.in_proj_weight", "attention.out_proj.weight", "ff_self.1.weight", "ff_self.3.weight")
V_NAMES = ("ln.weight", "ln.bias", "attention.in_proj_bias", "attention.out_proj.bias", "ff_self.0.weight", "ff_self.0.bias",
           "ff_self.1.bias", "ff_self.3.bias")
TAKES = {"fused64": ((0, 1, 2, 3), tuple(range(8))), "qkv": ((0,), (0, 1, 2)), "head": ((0,), (0, 1, 2)),
         "tail": ((1, 2, 3), (3, 4, 5, 6, 7)), "core": ((), ())}
_DEV = {}


def _lib():
    from state_policy_diffusionmodel_amd import _lib as L
    return L, L.load()


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype).reshape(-1)).cuda()


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float32, device="cuda")


def film_coef_dev(inp):
    """ab [B 2C] of the case's FilmSpec as the FILM_COEF stream op writes it"""
    L, lib = _lib()
    f, B, C = inp["film"], inp["B"], inp["C"]
    a = L.SpdmOpStreamArgs()
    a.op = L.OP_STREAM_OPS.index("film_coef")
    for i, v in enumerate((B, inp["L"], C, len(f["t"]), f["T"])):
        a.dim[i] = v
    temb, film, ab = _cuda(f["temb"]), _cuda(f["film"]), _nan(B * 2 * C)
    for i, t in enumerate((temb, film, ab)):
        a.d_buf[i], a.cap[i] = t.data_ptr(), t.numel()
    t = np.ascontiguousarray(f["t"], np.int32)
    a.h_idx[0], a.n_idx[0] = t.ctypes.data, t.size
    keep = _gn(a.gn[0], f["gn"])
    L.check(lib.spdm_op_stream(ctypes.byref(a)), "spdm_op_stream(film_coef)")
    del keep
    return ab


def _gn(dst, g):
    st, ga, be = _cuda(g["stats"], np.float64), _cuda(g["gamma"]), _cuda(g["beta"])
    dst.d_stats, dst.stats_cap = st.data_ptr(), st.numel()
    dst.slots, dst.m_tile, dst.n_tiles, dst.cnorm = g["slots"], g["m_tile"], g["n_tiles"], g["cnorm"]
    dst.d_gamma, dst.d_beta, dst.affine_cap = ga.data_ptr(), be.data_ptr(), ga.numel()
    return st, ga, be


def op_sa(op, inp, *, bufs, aff="own", ab_dev=None, no_wlds=0, expect_refusal=False):
    """One launch.  bufs: the op's device tensors in d_buf order (None: absent).  aff: 'own' (the case's ab or FilmSpec), 'ab'
    (ab_dev instead of the case's FilmSpec) or None.  Returns info (None when the hook refused and that was expected)."""
    L, lib = _lib()
    a = L.SpdmOpSaArgs()
    a.op = L.OP_SA_OPS.index(op)
    C, B, Ln = inp["C"], inp["B"], inp["L"]
    if op == "fused64":
        c = inp.get("crop")
        dims = (B, Ln, no_wlds) + ((1, c["H0"], c["D"], c["Wp"], c["lh"], c["lw"], 1 if inp.get("outc") else 0) if c else (0,) * 7)
    elif op == "core":
        dims = (B, Ln, C, inp["valu"])
    else:
        dims = (C, B, Ln)
    for i, v in enumerate(dims):
        a.dim[i] = v
    for i, t in enumerate(bufs):
        if t is not None:
            a.d_buf[i], a.cap[i] = t.data_ptr(), t.numel()
    keep = []
    wi, vi = TAKES[op]
    for i in wi:
        w = np.ascontiguousarray(inp["W"][W_NAMES[i]], np.float32)
        keep.append(w)
        a.h_w[i] = w.ctypes.data
    for i in vi:
        key = (id(inp["W"]), i)
        if key not in _DEV:
            _DEV[key] = _cuda(inp["W"][V_NAMES[i]])
        a.d_vec[i], a.vec_cap[i] = _DEV[key].data_ptr(), _DEV[key].numel()
    if aff == "ab" or (aff == "own" and inp.get("ab") is not None):
        ab = ab_dev if aff == "ab" else _cuda(inp["ab"])
        keep.append(ab)
        a.d_ab, a.ab_cap = ab.data_ptr(), ab.numel()
    elif aff == "own" and inp.get("film") is not None:
        f = inp["film"]
        a.film_on, a.t_count, a.T = 1, len(f["t"]), f["T"]
        temb, film, t = _cuda(f["temb"]), _cuda(f["film"]), np.ascontiguousarray(f["t"], np.int32)
        keep += [temb, film, t, _gn(a.gn, f["gn"])]
        a.d_temb, a.temb_cap, a.h_t, a.d_film, a.film_cap = temb.data_ptr(), temb.numel(), t.ctypes.data, film.data_ptr(), film.numel()
    if inp.get("outc") is not None:
        ow = _cuda(inp["outc"][0])
        keep.append(ow)
        a.d_outc_w, a.outc_w_cap, a.outc_b = ow.data_ptr(), 64, inp["outc"][1]
    torch.cuda.synchronize()
    rc = lib.spdm_op_sa(ctypes.byref(a))
    if rc not in (0, L.SPDM_ERR_INVALID):                                      # a device error: nothing more is launched on it
        pytest.exit(f"spdm_op_sa({op}) failed ({rc}): {lib.spdm_last_error().decode()}", returncode=3)
    if expect_refusal:
        assert rc == L.SPDM_ERR_INVALID, "the hook accepted a launch it must refuse"
        return None
    L.check(rc, f"spdm_op_sa({op})")
    return dict(zip(("kernel", "waves", "grid", "wlds", "qw"), (L.OP_SA_KERNELS[a.info[0]],) + tuple(a.info[1:5])))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def expected_route(op, inp):
    """what the case was written for, restated from the launchers' rules (csrc/sa_fused.hip, sa_tail.hip, attention.hip)"""
    C, B, L = inp["C"], inp["B"], inp["L"]
    TM, rows = 8192 // C, B * L
    tiles = -(-rows // TM)
    if op == "fused64":
        if inp.get("crop"):
            c, nw = inp["crop"], R.crop_waves(L)
            return dict(kernel="crop", waves=nw, grid=B, wlds=0, qw=-(-c["H0"] * c["D"] // nw))
        if L > 256:
            return dict(kernel="fused_pair", waves=8, grid=2 * B, wlds=0)
        nw = -(-L // 32)
        return dict(kernel="fused", waves=nw, grid=min(B, _cus()) if nw >= 4 else B, wlds=int(nw >= 4))
    if op == "qkv":
        return dict(kernel="qkv", waves=4, grid=3 * tiles)
    if op in ("head", "tail"):
        return dict(kernel=op, waves=4, grid=tiles)
    d, pairs = C // 4, 4 * B
    if L >= 32 and not inp["valu"]:
        return dict(kernel="core_mfma", waves=min(4, -(-L // 32)), grid=pairs * -(-L // 128))
    pow2 = L & (L - 1) == 0
    if L <= 16 and pow2 and d in (32, 64):
        return dict(kernel="core_ds", waves=4, grid=-(-pairs // (64 // L)))
    G = 64 // L if L <= 32 and pow2 else 1
    return dict(kernel="core_valu", waves=1 if G > 1 else min(4, -(-L // 64)), grid=-(-pairs // G))


def _run(op, inp, **kw):
    """(got {name: float64 array of the compared samples}, info, raw bytes of every output)"""
    C, B, L = inp["C"], inp["B"], inp["L"]
    sub = R.subset(inp)
    if op == "fused64":
        c = inp.get("crop")
        outc = inp.get("outc") is not None
        out = None if outc else _nan(B * L * 64)
        eps = _nan(B * c["H0"] * c["D"]) if outc else None
        info = op_sa(op, inp, bufs=(_cuda(inp["x"]), out, eps), **kw)
        if outc:
            e = eps.cpu().numpy()
            return {"eps": e.reshape(B, c["H0"], c["D"])[sub].astype(np.float64)}, info, e.tobytes()
        o = out.cpu().numpy()
        full = o.reshape(B, L, 64)
        if c is None:
            return {"out": full[sub].astype(np.float64)}, info, o.tobytes()
        tok = R.crop_tokens(c)
        rest = np.setdiff1d(np.arange(L), tok)
        assert np.isnan(full[:, rest]).all(), "the cropped launch wrote a token outside the crop"
        return {"out": full[sub][:, tok].astype(np.float64)}, info, o.tobytes()
    if op == "core":
        out = _nan(B * L * C)
        info = op_sa(op, inp, bufs=(_cuda(inp["qkv"]), out, None), aff=None)
    elif op == "tail":
        out = _nan(B * L * C)
        info = op_sa(op, inp, bufs=(_cuda(inp["att"]), _cuda(inp["x"]), out), **kw)
    else:
        out = _nan(B * L * (3 * C if op == "qkv" else C))
        info = op_sa(op, inp, bufs=(_cuda(inp["x"]), out, None), **kw)
    o = out.cpu().numpy()
    return {"out": o.reshape(B, L, -1)[sub].astype(np.float64)}, info, o.tobytes()


def _check(op, cid, inp, bd=None):
    ref = R.ref64(op, inp)
    bd = R.bound(op, inp, None if op == "fused64" else R.golden_tau(op, cid)) if bd is None else bd
    got, info, raw = _run(op, inp)
    assert set(got) == set(ref)
    ratio = R.worst_ratio(got, ref, bd)
    print(f"RATIO {op} {cid} {ratio:.4f}")
    want = expected_route(op, inp)
    assert {k: info[k] for k in want} == want, (info, want)
    for v in got.values():
        assert np.isfinite(v).all(), "an element the launch should write is not finite"
    assert ratio <= 1.0, f"{op} {cid}: error / bound = {ratio:.3f}"
    assert _run(op, inp)[2] == raw, "two launches on the same inputs differ"
    if inp.get("film") is not None:                                          # the recipe must equal its coefficients from memory
        assert _run(op, inp, aff="ab", ab_dev=film_coef_dev(inp))[2] == raw, "FilmSpec and ab (FILM_COEF) differ"
    if info["wlds"] == 1:
        again, info2, raw2 = _run(op, inp, no_wlds=1)
        assert info2["wlds"] == 0 and info2["grid"] == inp["B"]
        assert raw2 == raw, "wlds and no_wlds differ"


ALL = [(op, case) for op in R.OPS for case in R.cases(op)]


@pytest.mark.parametrize("op,case", ALL, ids=[f"{op}-{case[0]}" for op, case in ALL])
def test_launch_against_fp64(op, case):
    inp = R.make_inputs(op, case)
    if inp.get("refused"):                                                    # beyond 160 KiB of LDS: refused, nothing launches
        out = _nan(inp["B"] * inp["L"] * inp["C"])
        assert op_sa(op, inp, bufs=(_cuda(inp["qkv"]), out, None), aff=None, expect_refusal=True) is None
        assert torch.isnan(out).all()
        return
    _check(op, case[0], inp)


_KEEP = []


def _refused(op, spec, huge_weight=None):
    inp = R.make_inputs(op, ("refusal", spec))
    if huge_weight:                                                          # outside the split format's range, |w| < 511
        inp["W"] = {k: v.copy() for k, v in inp["W"].items()}
        inp["W"][huge_weight][1, 2] = 600.0
        _KEEP.append(inp["W"])                                               # (op_sa keys its device vectors by this dict)
    C, B, L = inp["C"], inp["B"], inp["L"]
    out = _nan(B * L * 3 * C)
    if op == "fused64":
        outc = inp.get("outc") is not None
        bufs = (_cuda(inp["x"]), None if outc else out, _nan(B * L) if outc else None)
    elif op == "core":
        bufs = (_cuda(inp["qkv"]), out, None)
    elif op == "tail":
        bufs = (_cuda(inp["att"]), _cuda(inp["x"]), out)
    else:
        bufs = (_cuda(inp["x"]), out, None)
    assert op_sa(op, inp, bufs=bufs, aff=None if op == "core" else "own", expect_refusal=True) is None
    assert torch.isnan(out).all(), "a refused launch wrote"


def test_refusals_launch_nothing():
    _refused("fused64", dict(B=2, L=320, aff="ab"))                          # the two-workgroup form takes no affine
    _refused("fused64", dict(B=3, L=320, aff="film", t_count=3))
    _refused("fused64", dict(B=2, L=64, crop=(8, 8, 8, 0, 0), outc=0))       # Q = L
    _refused("fused64", dict(B=2, L=256, crop=(27, 5, 8, 0, 0), outc=0))     # Q = 135 above the cap 128 (32 x 4 waves)
    _refused("fused64", dict(B=2, L=192, crop=(26, 5, 5, 0, 0), outc=1))     # Q = 130, the same with outc
    _refused("fused64", dict(B=2, L=64, crop=(4, 3, 8, 5, 0), outc=0))       # (lh + H0) Wp = 72 > L
    for C in (128, 256):
        _refused("qkv", dict(C=C, B=40, L=2, aff="film", t_count=1))         # sa_tail_film_local's 24 KiB
        _refused("tail", dict(C=C, B=40, L=2, aff="film", t_count=1))
        _refused("head", dict(C=C, B=3, L=3))                                # L does not divide the tile
        _refused("head", dict(C=C, B=3, L=8192 // C * 2))
    _refused("core", dict(C=256, B=3, L=320, valu=1, data="randn"))          # the VALU kernel beyond 160 KiB of LDS


def test_a_weight_outside_the_split_range_is_refused_as_the_plan_refuses_it():
    """the loader's range check (answered by the device) gives such a weight no split copy: the hook refuses and launches nothing"""
    _refused("fused64", dict(B=2, L=16), huge_weight="attention.in_proj_weight")          # perm_split (C = 64)
    _refused("fused64", dict(B=2, L=16), huge_weight="ff_self.3.weight")
    _refused("qkv", dict(C=128, B=3, L=5, aff="ab"), huge_weight="attention.in_proj_weight")   # linear_frag (C = 128 / 256)
    _refused("tail", dict(C=256, B=3, L=5, aff="ab"), huge_weight="ff_self.1.weight")


@pytest.mark.parametrize("route,C", R.CHAINS)
def test_chain(route, C):
    """Each launch is fed the previous launch's device output; the chain's output meets sa_bound, and each link alone its TAU_op on
    the inputs it actually received (TAU_op from the references, on those inputs)."""
    first, cid, inp = R.chain_inputs(route, C)
    blk = R._block64(inp, inp["x"], R.coefficients(inp))

    def link(op, li):
        ref, bd = R.ref64(op, li), R.bound(op, li)
        got, info, raw = _run(op, li)
        ratio = R.worst_ratio(got, ref, bd)
        print(f"RATIO {op} chain_{cid} {ratio:.4f}")
        assert info["kernel"] == expected_route(op, li)["kernel"]
        assert ratio <= 1.0, f"{op} in {cid}: error / bound = {ratio:.3f}"
        assert _run(op, li)[2] == raw
        return got["out"].astype(np.float32)

    if first == "qkv":
        qkv = link("qkv", inp)
        att = link("core", {**inp, "qkv": qkv, "valu": 0, "W": None, "ab": None, "film": None})
    else:
        att = link("head", inp)
    out = link("tail", {**inp, "att": att})
    ratio = float((np.abs(out.astype(np.float64) - blk["out"]) / blk["bound"]).max())
    print(f"RATIO chain {cid} {ratio:.4f}")
    assert ratio <= 1.0, f"{cid}: error / sa_bound = {ratio:.3f}"
