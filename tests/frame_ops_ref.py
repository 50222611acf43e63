"""Plain CPU references of ONE launch of the observation encoder / the autoencoder's decoder (spdm_op_frame, include/spdm.h), for
tests only: numpy, nothing from the project.  The contract is that of tests/train_ops_ref.py (ref64, scale64, ref32, MUTANTS,
cases, make_inputs; |got - ref64| <= TAU * S per element with TAU = 4 x ref32's own worst error in units of S, equality where S is
zero); its helpers are imported, as tests/stream_ops_ref.py does.

Rules of S particular to this family:
  (r - t) counts |r| + |t|, (1 - r) counts 1 + |r|;
  a factor that holds r, the output of the sigmoid, counts + TINY (DEC_BWD6: r may be subnormal);
  the sigmoid's S is its own value, plus its slope times the S of its argument (the argument is a computed sum here, not a
  leaf), plus TINY:  S(recon) = r (1 + sigmoid(-z) S(z)) + TINY;
  an ENC_X2 unit that is on counts the smallest normal number beside the S of its sum (the kernel never stores less).

The kink kernels, the masked permutations, the layout permutations and ADD are exact: their references return the float32
values the kernel must store, S is zero everywhere and the GPU test also compares the bits.

sq and loss are formed in float64 on the device and have references and tolerances of their own (sq_refs, loss_refs): the
float64 formula on the float32 reconstruction, TAU from a model that takes the float32 difference the kernel takes and a
SEQUENTIAL float64 sum.
"""
import math

import numpy as np

import train_ops_ref as T
from train_ops_ref import F32, F64, TINY, U, _randn, _seed, mm_t, ssum, worst_ratio  # noqa: F401

OPS = ("enc_convs", "enc_kinks", "enc_x2", "enc_dz3", "enc_dz2", "enc_conv1_wgrad", "add", "dec_convs", "dec_kinks", "dec_loss",
       "dec_bwd6", "dec_dgrad4", "dec_colsum", "dec_unperm_conv", "dec_unperm_linear", "frame_wgrad")
# ops whose reference is the exact float32 result (S = 0 everywhere): the GPU test compares bits as well
EXACT = ("enc_kinks", "enc_dz3", "enc_dz2", "add", "dec_kinks", "dec_unperm_conv", "dec_unperm_linear")
KINK = np.float32(1.17549435e-38)                 # what a kink kernel stores for a unit that is on and was saved as off
SUBNORMAL = np.float32(1e-45)
PIX = 3 * 96 * 96
CHUNK = 2048                                      # frames of one chunk of the two passes
ENC_W1_ROWS = 1024                                # rows of a workgroup of conv 1's weight gradient
ENC_WG_FLOATS = 8 * 128 * 9216                    # the slab budgets the passes hand to launch_wgrad (restated for the geometry)
DEC_WG_FLOATS = 8 * 128 * 9216
DEC_WG_SLABS = 256
# (Co, Ci, budget in floats, rows per frame) of FRAME_WGRAD's `which`
FRAME_WG = ((128, 9216, ENC_WG_FLOATS, 1), (64, 128, ENC_WG_FLOATS, 144), (32, 64, ENC_WG_FLOATS, 576),
            (32, 64, DEC_WG_SLABS * 32 * 64, 576), (64, 128, DEC_WG_SLABS * 64 * 128, 144), (9216, 128, DEC_WG_FLOATS, 1))

# Floors of TAU in units of u: roundings on the longest chain of one element beside its sums (which ref32 carries)
FLOOR_U = {
    # -z (0), expf (1 ulp = 2), 1 + (1), 1 / (1)
    "dec_convs": 4,
    # r - t (1), scale * (1), 1 - r (1), r * (1), the product (1); no math-library call
    "dec_bwd6": 5,
}
FLOOR_LOSS_U = 1                                  # the float32 store of the loss
FLOOR_SQ_U64 = 2                                  # float64: the last add and one for d d (exact for 24-bit d: kept as a margin)


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def rows_to_nchw(rows, n, levels, swap=None):
    """[n 144 4^levels][C] rows in the nested order (frame, qy, qx, ky1, kx1, ky2, kx2, ...) -> (n, C, 12 2^levels, ...) with the
    pixel at y = 2^levels qy + ... + ky_levels.  swap: two axes of the nested view exchanged first (a mutant's order)."""
    C = rows.shape[1]
    x = rows.reshape([n, 12, 12] + [2, 2] * levels + [C])
    if swap:
        x = np.swapaxes(x, *swap)
    ys = [1] + [3 + 2 * i for i in range(levels)]
    xs = [2] + [4 + 2 * i for i in range(levels)]
    side = 12 * 2 ** levels
    return x.transpose([0, x.ndim - 1] + ys + xs).reshape(n, C, side, side)


def nchw_to_rows(img, levels):
    """the inverse of rows_to_nchw"""
    n, C = img.shape[:2]
    x = img.reshape([n, C, 12] + [2] * levels + [12] + [2] * levels)           # n C qy ky1.. qx kx1..
    perm = [0, 2, 3 + levels] + [a for i in range(levels) for a in (3 + i, 4 + levels + i)] + [1]
    return x.transpose(perm).reshape(-1, C)


def dec_kernel_layout(sd):
    """torch-layout decoder tensors -> the layouts the launchers read: a transposed convolution (cin, cout, 2, 2) as
    [ci][kk][co], the Linear's rows and bias from Flatten order c 144 + q to q 64 + c."""
    K = {"w0": sd["0.weight"].reshape(64, 144, 128).transpose(1, 0, 2).reshape(9216, 128),
         "b0": sd["0.bias"].reshape(64, 144).T.reshape(9216)}
    for k, name in (("2", "2"), ("4", "4"), ("6", "6")):
        w = sd[k + ".weight"]
        K["w" + name] = w.transpose(0, 2, 3, 1).reshape(w.shape[0], 4, w.shape[1])
        K["b" + name] = sd[k + ".bias"]
    return {k: np.ascontiguousarray(v, F32) for k, v in K.items()}


def colsum_geometry(M):
    """(slab_rows, slabs) of launch_decoder_colsum: at most 256 slabs of at least 64 rows, rows a multiple of 4"""
    r = max(64, (M + 255) // 256)
    r = (r + 3) // 4 * 4
    return r, (M + r - 1) // r


def frame_wgrad_geometry(M, which):
    """(chunks, rows per chunk) wgrad_chunks gives for taps 1 under the budget of `which`"""
    Co, Ci, budget, _ = FRAME_WG[which]
    tiles = ((Co + 63) // 64) * ((Ci + 63) // 64)
    n = max(1, 2048 // tiles)
    n = min(n, max(1, M // 64))
    n = min(n, max(1, budget // (Co * Ci)))
    rows = (M + n - 1) // n
    return n, (rows + 3) // 4 * 4


def conv1_wgrad_blocks(n):
    return (n * 576 + ENC_W1_ROWS - 1) // ENC_W1_ROWS


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _V(inp, dt, ab, *names):
    out = []
    for n in names:
        v = np.asarray(inp[n]).astype(dt)
        out.append(np.abs(v) if ab else v)
    return out


def lin(x, w, b, seq):
    """x [R][K] w [K][N] + b [N]: the bias first, then k ascending; seq: one rounded product and one rounded add per k"""
    if not seq:
        return x @ w + (0 if b is None else b)
    acc = np.zeros((x.shape[0], w.shape[1]), x.dtype)
    if b is not None:
        acc += b
    for k in range(x.shape[1]):
        acc += x[:, k:k + 1] * w[k:k + 1, :]
    return acc


def _sig(z):
    with np.errstate(over="ignore"):
        return (1 / (1 + np.exp(-z))).astype(z.dtype)


def _relu(x, ab):
    return x if ab else np.maximum(x, 0)


def kink_fix(a32, pre64):
    """what a kink kernel leaves of a saved float32 activation given the float64 pre-activation"""
    a32 = np.asarray(a32, F32)
    on = pre64 > 0
    return np.where(on == (a32 > 0), a32, np.where(on, KINK, F32(0))).astype(F32)


# ---- the encoder -----------------------------------------------------------------------------------------------------------
def _padded(img, mutant):
    """P[n, c, Y, X] = img[n, c, Y - 1, X - 1] for Y, X in 0..95, zero outside the image (conv 1's padding; its row / column 48
    is never read).  Mutants: the bound left out (flat memory read instead), the origin without the - 1."""
    n = img.shape[0]
    if mutant == "origin_4py":
        return img.copy()
    P = np.zeros_like(img)
    P[:, :, 1:, 1:] = img[:, :, :95, :95]
    if mutant == "no_zero_border":
        flat = img.ravel()
        Y, X = np.meshgrid(np.arange(96), np.arange(96), indexing="ij")
        base = (np.arange(n * 3) * 9216).reshape(n, 3, 1, 1)
        P = flat[(base + (Y - 1) * 96 + (X - 1)) % flat.size]
    return P


def _patches12(P):
    """[n][48][48][c 4 + jy 2 + jx]: conv 1's input vectors at its positions 0..47"""
    n = P.shape[0]
    return P.reshape(n, 3, 48, 2, 48, 2).transpose(0, 2, 4, 1, 3, 5).reshape(n, 48, 48, 12)


def _s2d(a):
    """[n][2H][2W][C] -> [n][H][W][c 4 + ky 2 + kx]"""
    n, H2, W2, C = a.shape
    return a.reshape(n, H2 // 2, 2, W2 // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(n, H2 // 2, W2 // 2, C * 4)


def _x2_rows(a):
    """[n][48][48][C] by conv-1 position -> x2's rows [(n 144 + q) 4 + kk][c 4 + ky 2 + kx] (kk: conv-2 position in window q)"""
    n, C = a.shape[0], a.shape[3]
    v = a.reshape(n, 12, 2, 2, 12, 2, 2, C)                                    # n qy kyq ky qx kxq kx c
    return v.transpose(0, 1, 4, 2, 5, 7, 3, 6).reshape(n * 576, C * 4)


def enc_forward(inp, dt, ab, seq, mutant=None):
    """the three convolutions: conv-1 map by position [n][48][48][16] (pre and post), x3 rows (pre and post), feat rows (pre)"""
    img, w1, b1, w2, b2, w3, b3 = _V(inp, dt, ab, "img", "w1", "b1", "w2", "b2", "w3", "b3")
    n = img.shape[0]
    p12 = _patches12(_padded(img, mutant))
    pre1 = lin(p12.reshape(-1, 12), w1.reshape(16, 12).T, b1, seq).reshape(n, 48, 48, 16)
    a1 = _relu(pre1, ab)
    pre2 = lin(_s2d(a1).reshape(-1, 64), w2.reshape(32, 64).T, b2, seq).reshape(n, 24, 24, 32)
    a2 = _relu(pre2, ab)
    x3pre, x3 = _s2d(pre2).reshape(n * 144, 128), _s2d(a2).reshape(n * 144, 128)
    if mutant == "x3_kykx_swapped":
        x3 = x3.reshape(-1, 32, 2, 2).transpose(0, 1, 3, 2).reshape(-1, 128)
    pre3 = lin(_s2d(a2).reshape(n * 144, 128), w3.reshape(64, 128).T, b3, seq)                # [n 144][64]
    return {"pre1": pre1, "a1": a1, "x3pre": x3pre, "x3": x3, "pre3": pre3}


def _flatten_order(rows, n):
    """[n 144][64] -> [n][co 144 + q]"""
    return rows.reshape(n, 144, 64).transpose(0, 2, 1).reshape(n, 9216)


def _enc_convs(inp, dt, ab, seq, mutant):
    f = enc_forward(inp, dt, ab, seq, mutant)
    n = np.asarray(inp["img"]).shape[0]
    out = {"feat": _flatten_order(_relu(f["pre3"], ab), n)}
    if inp["train"]:
        out["x3"] = f["x3"]
    return out


def _enc_kinks(inp, dt, ab, seq, mutant):
    n = np.asarray(inp["img"]).shape[0]
    if ab:
        return {"feat": np.zeros((n, 9216), dt), "x3": np.zeros((n * 144, 128), dt)}
    f = enc_forward(inp, F64, False, False)
    return {"feat": kink_fix(inp["feat"], _flatten_order(f["pre3"], n)), "x3": kink_fix(inp["x3"], f["x3pre"])}


def _enc_x2(inp, dt, ab, seq, mutant):
    f = enc_forward(inp, dt, ab, seq, mutant)
    on = _x2_rows(enc_forward(inp, F64, False, False, mutant)["pre1"]) > 0     # the sign comes from float64 in every precision
    if ab:
        return {"x2": np.where(on, _x2_rows(f["pre1"]) + float(KINK), 0.0)}
    return {"x2": np.where(on, np.maximum(_x2_rows(f["pre1"]), dt(KINK)), dt(0)).astype(dt)}


def _mask(a, mutant):
    a = np.asarray(a, F32)
    return a >= 0 if mutant == "mask_ge" else a > 0


def _enc_dz3(inp, dt, ab, seq, mutant):
    n = inp["feat"].shape[0]
    if ab:
        return {"dz3": np.zeros((n * 144, 64), dt)}
    g = np.where(_mask(inp["feat"], mutant), np.asarray(inp["dfeat"], F32), F32(0))
    if mutant == "transposed":
        return {"dz3": g.reshape(n * 144, 64)}
    return {"dz3": g.reshape(n, 64, 144).transpose(0, 2, 1).reshape(n * 144, 64)}


def _enc_dz2(inp, dt, ab, seq, mutant):
    R = inp["x3"].shape[0]
    if ab:
        return {"dz2": np.zeros((R, 128), dt)}
    g = np.where(_mask(inp["x3"], mutant), np.asarray(inp["dx3"], F32), F32(0))
    if mutant == "transposed":
        return {"dz2": g}
    return {"dz2": g.reshape(R, 32, 4).transpose(0, 2, 1).reshape(R, 128)}    # [nq][kk 32 + ci]: rows nq 4 + kk of 32


def _enc_conv1_wgrad(inp, dt, ab, seq, mutant):
    img, dx2 = _V(inp, dt, ab, "img", "dx2")
    n = img.shape[0]
    rows = n * 576
    g = np.where(_mask(inp["x2"], mutant), dx2, 0).astype(dt).reshape(rows, 16, 4)          # [row][c1][kk]
    if mutant == "drop_last_block":
        g[rows // ENC_W1_ROWS * ENC_W1_ROWS:] = 0
    p = _x2_rows(_patches12(_padded(img, None))).reshape(rows, 12, 4)                         # [row][c 4 + j][kk]
    dw = np.zeros((16, 12), dt)
    gb = g[:, :, :3] if mutant == "bias_kk_missing" else g
    if seq:
        for kk in range(4):
            dw += mm_t(g[:, :, kk], p[:, :, kk], True)
        db = ssum(gb.transpose(1, 0, 2), (1, 2), True)
    else:
        dw = np.einsum("rak,rck->ac", g, p)
        db = gb.sum((0, 2))
    return {"dw": dw.reshape(192), "db": db}


def _add(inp, dt, ab, seq, mutant):
    if ab:
        return {"dst": np.zeros(inp["src"].shape, dt)}
    if mutant == "assign":
        return {"dst": np.asarray(inp["src"], F32)}
    return {"dst": (np.asarray(inp["dst"], F32) + np.asarray(inp["src"], F32)).astype(F32)}    # one float32 add


# ---- the decoder -----------------------------------------------------------------------------------------------------------
def dec_layers(h0, w2, b2, w4, b4, w6, b6, ab, seq):
    """h0 [n 144][64] -> pre1 [n 576][32], pre2 [n 2304][16], z6 [n 9216][3] (rows r2, r3, r4 of csrc/decoder.hip)"""
    pre1 = lin(h0, w2.reshape(64, 128), np.tile(b2, 4), seq).reshape(-1, 32)
    pre2 = lin(_relu(pre1, ab), w4.reshape(32, 64), np.tile(b4, 4), seq).reshape(-1, 16)
    z6 = lin(_relu(pre2, ab), w6.reshape(16, 12), np.tile(b6, 4), seq).reshape(-1, 3)
    return pre1, pre2, z6


def _dec_convs(inp, dt, ab, seq, mutant):
    h0, w2, b2, w4, b4, w6, b6 = _V(inp, dt, ab, "h0", "w2", "b2", "w4", "b4", "w6", "b6")
    n = h0.shape[0] // 144
    pre1, pre2, z6 = dec_layers(h0, w2, b2, w4, b4, w6, b6, ab, seq)
    swap = {"recon_ky2_ky3": (5, 7), "scatter_kykx": (3, 4)}.get(mutant)
    if ab:
        z = dec_layers(*_V(inp, dt, False, "h0", "w2", "b2", "w4", "b4", "w6", "b6"), False, False)[2]
        recon = _sig(z) * (1 + _sig(-z) * z6) + TINY
    else:
        recon = _sig(z6)
    out = {"recon": rows_to_nchw(recon, n, 3, swap)}
    if inp["train"]:
        out["a1"], out["a2"] = _relu(pre1, ab), _relu(pre2, ab)
    return out


def dec_pre64(inp):
    """float64 pre-activations of the two ReLU layers from the latents"""
    lat, w0, b0, w2, b2, w4, b4 = _V(inp, F64, False, "latent", "w0", "b0", "w2", "b2", "w4", "b4")
    h0 = (lat @ w0.T + b0).reshape(-1, 64)
    pre1 = lin(h0, w2.reshape(64, 128), np.tile(b2, 4), False).reshape(-1, 32)
    pre2 = lin(np.maximum(pre1, 0), w4.reshape(32, 64), np.tile(b4, 4), False).reshape(-1, 16)
    return h0, pre1, pre2


def _dec_kinks(inp, dt, ab, seq, mutant):
    if ab:
        return {"a1": np.zeros(inp["a1"].shape, dt), "a2": np.zeros(inp["a2"].shape, dt)}
    _, pre1, pre2 = dec_pre64(inp)
    return {"a1": kink_fix(inp["a1"], pre1), "a2": kink_fix(inp["a2"], pre2)}


def kink_margin(op, inp):
    """min over every ReLU unit the kink op decides of |pre64| / S(pre64)"""
    a = lambda *k: _V(inp, F64, True, *k)
    if op == "dec_kinks":
        _, pre1, pre2 = dec_pre64(inp)
        lat, w0, b0, w2, b2, w4, b4 = a("latent", "w0", "b0", "w2", "b2", "w4", "b4")
        s1 = lin((lat @ w0.T + b0).reshape(-1, 64), w2.reshape(64, 128), np.tile(b2, 4), False).reshape(-1, 32)
        s2 = lin(s1, w4.reshape(32, 64), np.tile(b4, 4), False).reshape(-1, 16)
        pairs = [(pre1, s1), (pre2, s2)]
    else:
        f, s = enc_forward(inp, F64, False, False), enc_forward(inp, F64, True, False)
        pairs = [(f["pre1"], s["pre1"])] if op == "enc_x2" else [(f["x3pre"], s["x3pre"]), (f["pre3"], s["pre3"])]
    return min(float((np.abs(p) / s).min()) for p, s in pairs)


def _dec_bwd6(inp, dt, ab, seq, mutant):
    r, t, a2, w6 = _V(inp, dt, ab, "recon", "target", "a2", "w6")
    scale = dt(abs(inp["scale"]) if ab else inp["scale"])
    if ab:
        g = (scale * (r + t) + TINY) * (r * (1 + r) + TINY)                   # r is a leaf out of exp: both factors count + TINY
    elif mutant == "no_sigmoid_slope":
        g = scale * (r - t)
    elif mutant == "slope_from_target":
        g = (scale * (r - t)) * (t * (1 - t))
    else:
        g = (scale * (r - t)) * (r * (1 - r))
    g = nchw_to_rows(g, 3).reshape(-1, 4, 3)                                   # [r3][kk3][co]
    gj = g.reshape(-1, 12)                                                     # column kk3 3 + co
    on = _mask(inp["a2"], mutant)
    dz4 = np.where(on, lin(gj, w6.reshape(16, 12).T, None, seq), 0).astype(dt)
    dw = mm_t(a2, gj, seq).reshape(16, 4, 3)                                   # [ci][kk3][co]
    if ab:
        dw = dw + TINY                     # a2 may sit at the edge of the normal range (planted): its products lie below it
    gb = g[:, :3] if mutant == "bias_kk_missing" else g
    db = ssum(gb.transpose(2, 0, 1), (1, 2), seq)
    return {"dz4": dz4, "dw": (dw if mutant == "dw_kernel_order" else dw.transpose(0, 2, 1)).reshape(192), "db": db}


def _dec_dgrad4(inp, dt, ab, seq, mutant):
    dz4, w4 = _V(inp, dt, ab, "dz4", "w4")
    w = w4.reshape(32, 64)                                                     # [ci][kk2 16 + co]
    if mutant == "j_order":
        w = w4.reshape(32, 4, 16).transpose(0, 2, 1).reshape(32, 64)           # read as co 4 + kk2
    return {"dz2": np.where(_mask(inp["a1"], mutant), lin(dz4, w.T, None, seq), 0).astype(dt)}


def _dec_colsum(inp, dt, ab, seq, mutant):
    (src,) = _V(inp, dt, ab, "src")
    M, C, fold = inp["M"], inp["C"], inp["fold"]
    src = src.copy()
    rows, slabs = colsum_geometry(M)
    if mutant == "drop_ragged_slab" and M % rows:
        src[(slabs - 1) * rows:] = 0
    if mutant == "drop_rows_3mod4":
        src[3::4] = 0
    s = ssum(src.T, 1, seq)
    if fold == 1:
        return {"dst": s if mutant == "fold1_transposed" else s.reshape(144, 64).T.reshape(C)}
    return {"dst": ssum(s.reshape(4, C // 4).T, 1, seq)}


def _dec_unperm_conv(inp, dt, ab, seq, mutant):
    cin, cout = inp["cin"], inp["cout"]
    if ab:
        return {"dst": np.zeros(cin * cout * 4, dt)}
    src = np.asarray(inp["src"], F32).reshape(cin, 4, cout)
    return {"dst": (src if mutant == "transposed" else src.transpose(0, 2, 1)).reshape(-1)}


def _dec_unperm_linear(inp, dt, ab, seq, mutant):
    if ab:
        return {"dst": np.zeros(9216 * 128, dt)}
    src = np.asarray(inp["src"], F32).reshape(144, 64, 128)
    return {"dst": (src if mutant == "transposed" else src.transpose(1, 0, 2)).reshape(-1)}


def _frame_wgrad(inp, dt, ab, seq, mutant):
    dy, x = _V(inp, dt, ab, "dy", "x")
    if mutant == "drop_chunk":
        nch, rows = frame_wgrad_geometry(inp["M"], inp["which"])
        c = 1 if nch > 1 else 0
        dy = dy.copy()
        dy[c * rows:min(inp["M"], (c + 1) * rows)] = 0
    return {"dst": mm_t(dy, x, seq)}


_IMPL = {"enc_convs": _enc_convs, "enc_kinks": _enc_kinks, "enc_x2": _enc_x2, "enc_dz3": _enc_dz3, "enc_dz2": _enc_dz2,
         "enc_conv1_wgrad": _enc_conv1_wgrad, "add": _add, "dec_convs": _dec_convs, "dec_kinks": _dec_kinks, "dec_bwd6": _dec_bwd6,
         "dec_dgrad4": _dec_dgrad4, "dec_colsum": _dec_colsum, "dec_unperm_conv": _dec_unperm_conv,
         "dec_unperm_linear": _dec_unperm_linear, "frame_wgrad": _frame_wgrad}

MUTANTS = {
    "enc_convs": ("no_zero_border", "origin_4py", "x3_kykx_swapped"),
    "enc_kinks": (),                                                           # (held by its own rule: test_kinks_*)
    "enc_x2": ("no_zero_border", "origin_4py"),
    "enc_dz3": ("mask_ge", "transposed"),
    "enc_dz2": ("mask_ge", "transposed"),
    "enc_conv1_wgrad": ("mask_ge", "drop_last_block", "bias_kk_missing"),
    "add": ("assign",),
    "dec_convs": ("recon_ky2_ky3", "scatter_kykx"),
    "dec_kinks": (),
    "dec_loss": ("divide_by_n", "first256"),
    "dec_bwd6": ("mask_ge", "bias_kk_missing", "no_sigmoid_slope", "slope_from_target", "dw_kernel_order"),
    "dec_dgrad4": ("mask_ge", "j_order"),
    "dec_colsum": ("drop_ragged_slab", "drop_rows_3mod4", "fold1_transposed"),
    "dec_unperm_conv": ("transposed",),
    "dec_unperm_linear": ("transposed",),
    "frame_wgrad": ("drop_chunk",),
}


# ---- sq and loss: float64 on the device ------------------------------------------------------------------------------------
def sq_refs(recon32, target, mutant=None):
    """The per-frame sums of squared errors on the float32 reconstruction: (ref64, S, model).  ref64 is the float64 formula
    (r - t exact in float64, math.fsum); S counts (|r| + |t|)^2; the model takes the kernel's float32 difference and a sequential
    float64 sum in pixel order.  Mutant: the sum taken in float32."""
    r, t = np.asarray(recon32, F32), np.asarray(target, F32)
    n = r.shape[0]
    d64 = r.astype(F64).reshape(n, -1) - t.astype(F64).reshape(n, -1)
    ref = np.array([math.fsum(row * row) for row in d64])
    S = np.array([math.fsum(row * row) for row in np.abs(r.astype(F64)).reshape(n, -1) + np.abs(t.astype(F64)).reshape(n, -1)])
    d32 = (r - t).reshape(n, -1)
    if mutant == "sum_in_float32":
        return ref, S, np.add.accumulate(d32 * d32, axis=1)[:, -1].astype(F64)
    d = d32.astype(F64)
    return ref, S, np.add.accumulate(d * d, axis=1)[:, -1]


def _own_tau(ref, S, model, floor):
    err = np.abs(model - ref)
    assert np.all(err[S == 0] == 0)
    worst = float((err[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0
    return max(4.0 * worst, floor) if (S > 0).any() else 0.0


def sq_tau(ref, S, model):
    return _own_tau(ref, S, model, FLOOR_SQ_U64 * 2.0 ** -53)


def loss_refs(sq, mutant=None):
    """loss = sum(sq) / (n 27648) stored as float32: (ref64 [1], S [1], model [1]); the model adds sequentially in float64."""
    sq = np.asarray(sq, F64)
    n = sq.size
    ref = math.fsum(sq) / (n * float(PIX))
    if mutant == "divide_by_n":
        return np.array([ref]), np.array([ref]), np.array([math.fsum(sq) / n])
    if mutant == "first256":
        return np.array([ref]), np.array([ref]), np.array([math.fsum(sq[:256]) / (n * float(PIX))])
    model = float(F32(np.add.accumulate(sq)[-1] / (n * float(PIX))))
    return np.array([ref]), np.array([ref]), np.array([model])


def loss_tau(ref, S, model):
    return _own_tau(ref, S, model, FLOOR_LOSS_U * U)


def _dec_loss(inp, dt, ab, seq, mutant):
    ref, S, model = loss_refs(inp["sq"], mutant)
    if ab:
        return {"loss": S}
    if mutant:
        return {"loss": model}
    return {"loss": model.astype(F32) if seq else ref}


_IMPL["dec_loss"] = _dec_loss


def ref64(op, inp, mutant=None):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        return {k: np.asarray(v, F64) for k, v in _IMPL[op](inp, F64, False, False, mutant).items()}


def scale64(op, inp):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        return {k: np.asarray(v, F64) for k, v in _IMPL[op](inp, F64, True, False, None).items()}


def ref32(op, inp):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        out = _IMPL[op](inp, F32, False, True, None)
    for k, v in out.items():
        assert np.asarray(v).dtype == F32, (op, k, np.asarray(v).dtype)
    return {k: np.asarray(v, F64) for k, v in out.items()}


def exact32(op, inp):
    """the float32 arrays an EXACT op must store, bit for bit"""
    assert op in EXACT
    return {k: np.asarray(v, F32) for k, v in _IMPL[op](inp, F64, False, False, None).items()}


def tau(op, inp, r64=None, s64=None):
    floors = dict(FLOOR_U, dec_loss=FLOOR_LOSS_U)
    return T.tau(op, inp, r64, s64, refs=(ref64, scale64, ref32, floors))


# ---- data ------------------------------------------------------------------------------------------------------------------
def _uniform(rng, shape, fan_in):
    b = 1.0 / math.sqrt(fan_in)
    return ((rng.random(shape) * 2 - 1) * b).astype(F32)


def enc_state(rng, flavour="init"):
    """encoder convolutions in torch layout (cout, cin, 2, 2), torch's default initialisation"""
    sd = {}
    for name, (co, ci) in (("1", (16, 3)), ("2", (32, 16)), ("3", (64, 32))):
        sd["w" + name], sd["b" + name] = _uniform(rng, (co, ci, 2, 2), ci * 4), _uniform(rng, (co,), ci * 4)
    if flavour in ("trained", "dead"):
        for k in ("w1", "w2", "w3"):
            sd[k] = (sd[k] * 3).astype(F32)
    if flavour == "dead":
        sd["b1"][[2, 9]] = -50
        sd["b2"][[3, 17, 31]] = -50
        sd["b3"][[4, 40, 63]] = -50
    if flavour == "alldead":
        sd["b2"][:] = -50                                                      # every conv-2 unit off
    return sd


def frames(rng, n, flavour="init"):
    x = rng.random((n, 3, 96, 96)).astype(F32)
    if flavour in ("trained", "dead"):
        x = (np.round(x * 255) / 255).astype(F32)                              # 8-bit frames
        x[:, :, 0:20, :] = 0                                                   # a black band that touches the padded border
        x[:, :, 40:60, 30:50] = 1                                              # a white patch
        x[:, :, 70:90, 60:90] = F32(128 / 255)                                 # a flat grey patch
    if flavour == "extreme":
        x[0] = 0                                                               # an all-black and an all-white frame
        x[-1] = 1
    return x


def dec_state(rng, flavour="init"):
    """decoder tensors in torch layout, torch's default initialisation (ConvTranspose2d: fan_in = cout 4)"""
    sd = {"0.weight": _uniform(rng, (9216, 128), 128), "0.bias": _uniform(rng, (9216,), 128)}
    for k, (ci, co) in (("2", (64, 32)), ("4", (32, 16)), ("6", (16, 3))):
        sd[k + ".weight"], sd[k + ".bias"] = _uniform(rng, (ci, co, 2, 2), co * 4), _uniform(rng, (co,), co * 4)
    if flavour == "dead":
        sd["2.bias"][[1, 7, 20]] = -50
        sd["4.bias"][[0, 5]] = -50
    if flavour == "a1dead":
        sd["2.bias"][:] = -50
    if flavour == "a2dead":
        sd["4.bias"][:] = -50
    return sd


def latents(rng, n):
    z = _randn(rng, n, 128, scale=0.3)
    z[-1] = 0
    return z


def dec_world(rng, n, flavour):
    """weights (kernel layout), latents, and the float64 forward of a decoder case.  trained40 / trained120 scale layer 6 by 40 /
    120 (recon from 1e-3 to 0.9996 / from 1e-9 to exactly 1.0f); extreme scales it until z6 reaches +120 and -110 (expf(-z)
    overflows below -88.7 and r is exactly 0; 1 + e is exactly 1 above 17.4)."""
    base = {"trained40": "init", "trained120": "init", "extreme": "init"}.get(flavour, flavour)
    sd = dec_state(rng, base)
    lat = latents(rng, n)
    K = dec_kernel_layout(sd)
    k6 = {"trained40": 40.0, "trained120": 120.0}.get(flavour, 1.0)
    if flavour == "extreme":
        z = dec_forward64(K, lat)["z6"]
        k6 = max(120.0 / z.max(), 110.0 / -z.min())
    K["w6"], K["b6"] = (K["w6"] * F32(k6)).astype(F32), (K["b6"] * F32(k6)).astype(F32)
    f = dec_forward64(K, lat)
    if flavour.startswith("trained"):
        target = (np.round(f["recon"] * 255) / 255).astype(F32)                # recon - target cancels to 8 bits
    else:
        target = rng.random((n, 3, 96, 96)).astype(F32)
        if flavour == "extreme":
            target[0] = 0
            target[-1] = 1
    return K, lat, f, target


def dec_forward64(K, lat):
    inp = dict(K, latent=lat)
    h0, pre1, pre2 = dec_pre64(inp)
    a2 = np.maximum(pre2, 0)
    z6 = lin(a2, K["w6"].astype(F64).reshape(16, 12), np.tile(K["b6"].astype(F64), 4), False).reshape(-1, 3)
    n = lat.shape[0]
    return {"h0": h0, "pre1": pre1, "a1": np.maximum(pre1, 0), "pre2": pre2, "a2": a2, "z6": z6,
            "recon": rows_to_nchw(_sig(z6), n, 3)}


def specials(a):
    """a saved activation map with +0.0, -0.0, the smallest normal and a subnormal planted: masks read them as off, off, on, on"""
    a = np.array(a, F32)
    f = a.reshape(-1)
    for k, v in enumerate((F32(0.0), F32(-0.0), KINK, SUBNORMAL)):
        f[k::11] = v
    return a


def saved_map(a32, how):
    a32 = np.asarray(a32, F32)
    return {"zeros": np.zeros_like(a32), "ones": np.ones_like(a32), "fwd": a32, "neg": -a32}[how]


FRAME_N = (1, 2, 3, 5)


def cases(op):
    """[(id, {flavour, ...})]"""
    C = []
    add = lambda cid, **kw: C.append((cid, kw))
    if op == "enc_convs":
        for train in (0, 1):
            for fl, n in (("init", 1), ("init", 3), ("trained", 2), ("dead", 2), ("alldead", 1), ("extreme", 2)):
                add(f"t{train}-{fl}-n{n}", flavour=fl, n=n, train=train)
    elif op in ("enc_kinks", "dec_kinks"):
        fls = ("init", "trained", "dead", "extreme") if op == "enc_kinks" else ("init", "trained120", "dead", "extreme")
        for how in ("zeros", "ones", "fwd", "neg"):
            for fl, n in zip(fls, (1, 2, 3, 2)):
                add(f"{how}-{fl}-n{n}", flavour=fl, n=n, saved=how)
        add("fwd-init-n5", flavour="init", n=5, saved="fwd")
    elif op == "enc_x2":
        for fl, n in (("init", 1), ("init", 3), ("trained", 2), ("dead", 5), ("extreme", 2)):
            add(f"{fl}-n{n}", flavour=fl, n=n)
    elif op in ("enc_dz3", "enc_dz2", "dec_dgrad4", "enc_conv1_wgrad", "dec_bwd6"):
        dead = {"dec_dgrad4": "a1dead", "dec_bwd6": "a2dead"}.get(op, "alldead")
        tr = ("trained40", "trained120") if op == "dec_bwd6" else ("trained",) if op.startswith("enc") else ("trained120",)
        table = [("init", n) for n in FRAME_N] + [(t, 2) for t in tr] + [("dead", 2), (dead, 1), ("extreme", 3), ("zero", 1)]
        for fl, n in table:
            add(f"{fl}-n{n}", flavour=fl, n=n)
    elif op == "add":
        for n in (1, 255, 256, 257):
            add(f"n{n}", flavour="init", n=n)
    elif op == "dec_convs":
        for train in (0, 1):
            for fl, n in (("init", 1), ("init", 3), ("trained40", 2), ("trained120", 2), ("dead", 2), ("a1dead", 1), ("extreme", 2)):
                add(f"t{train}-{fl}-n{n}", flavour=fl, n=n, train=train)
    elif op == "dec_loss":
        for n in (1, 255, 256, 257, 600):
            add(f"n{n}", flavour="init", n=n)
        add("n257-spread", flavour="spread", n=257)
    elif op == "dec_colsum":
        for Cc in (64, 128):
            for M in (1, 63, 64, 65, 130, 576, 16384, 16385):
                add(f"fold4-C{Cc}-M{M}", flavour="init", M=M, C=Cc, fold=4)
        for M in (1, 63, 64, 65, 130):
            add(f"fold1-M{M}", flavour="init", M=M, C=9216, fold=1)
    elif op == "dec_unperm_conv":
        for cin, cout in ((64, 32), (32, 16), (16, 3)):
            add(f"{cin}x{cout}", flavour="init", cin=cin, cout=cout)
    elif op == "dec_unperm_linear":
        add("w0", flavour="init")
    elif op == "frame_wgrad":
        for which in (0, 5):
            for M in (1, 3, 64, 130):
                add(f"w{which}-M{M}", flavour="init", which=which, M=M)
        for which in (1, 2, 3, 4):
            for n in (1, 2, 29, 30):
                add(f"w{which}-M{576 * n}", flavour="init", which=which, M=576 * n)
    else:
        raise KeyError(op)
    return C


def _enc_inputs(rng, fl, n):
    base = "init" if fl in ("zero",) else fl
    sd = enc_state(rng, "init" if base == "extreme" else base)
    inp = dict(sd, img=frames(rng, n, base), train=1)
    return inp


def make_inputs(op, case):
    cid, kw = case
    rng = np.random.default_rng(_seed("frame/" + op, cid))
    fl = kw["flavour"]
    inp = dict(kw)
    zero = fl == "zero"
    gscale = 0.0 if zero else 1e-3
    if op.startswith("enc"):
        n = kw["n"]
        inp.update(_enc_inputs(rng, fl, n))
        inp["train"] = kw.get("train", 1)
        if op in ("enc_convs", "enc_x2"):
            return inp
        f64 = enc_forward(inp, F64, False, False)
        f32 = enc_forward(inp, F32, False, True) if op == "enc_kinks" else None
        sp = specials if fl == "extreme" else (lambda a: a)
        if op == "enc_kinks":                                                  # the fp32 forward's own maps, flavoured
            inp["feat"] = saved_map(_flatten_order(np.maximum(f32["pre3"], 0), n), kw["saved"])
            inp["x3"] = saved_map(f32["x3"], kw["saved"])
        elif op == "enc_dz3":
            inp["feat"] = sp(_flatten_order(np.maximum(f64["pre3"], 0), n).astype(F32))
            inp["dfeat"] = _randn(rng, n, 9216, scale=gscale)
        elif op == "enc_dz2":
            inp["x3"] = sp(f64["x3"].astype(F32))
            inp["dx3"] = _randn(rng, n * 144, 128, scale=gscale)
        elif op == "enc_conv1_wgrad":
            inp["x2"] = sp(_x2_rows(f64["a1"]).astype(F32))
            inp["dx2"] = _randn(rng, n * 576, 64, scale=gscale)
        return inp
    if op == "add":
        inp["src"], inp["dst"] = _randn(rng, kw["n"]), _randn(rng, kw["n"])
        return inp
    if op == "dec_loss":
        n = kw["n"]
        sq = rng.random(n) * 2000 + 300                                        # a frame's sum: 27648 pixels of error ~0.3
        if fl == "spread":
            sq *= 10.0 ** rng.uniform(-6, 3, n)
        inp["sq"] = sq.astype(F64)
        return inp
    if op == "dec_colsum":
        inp["src"] = _randn(rng, kw["M"], kw["C"])
        return inp
    if op == "dec_unperm_conv":
        inp["src"] = _randn(rng, kw["cin"] * kw["cout"] * 4)
        return inp
    if op == "dec_unperm_linear":
        inp["src"] = _randn(rng, 9216 * 128)
        return inp
    if op == "frame_wgrad":
        Co, Ci = FRAME_WG[kw["which"]][:2]
        inp["dy"], inp["x"] = _randn(rng, kw["M"], Co), _randn(rng, kw["M"], Ci)
        return inp
    # the per-frame decoder ops
    n = kw["n"]
    K, lat, f, target = dec_world(rng, n, "init" if zero else fl)
    sp = specials if fl == "extreme" else (lambda a: a)
    if op == "dec_convs":
        inp.update({k: K[k] for k in ("w2", "b2", "w4", "b4", "w6", "b6")}, h0=f["h0"].astype(F32), target=target)
    elif op == "dec_kinks":
        inp.update(K, latent=lat)
        pre1, pre2, _ = dec_layers(f["h0"].astype(F32), *(K[k] for k in ("w2", "b2", "w4", "b4", "w6", "b6")), False, True)
        inp["a1"] = saved_map(np.maximum(pre1, 0), kw["saved"])
        inp["a2"] = saved_map(np.maximum(pre2, 0), kw["saved"])
    elif op == "dec_bwd6":
        inp.update(recon=f["recon"].astype(F32), target=target if not zero else f["recon"].astype(F32),
                   a2=sp(f["a2"].astype(F32)), w6=K["w6"].reshape(16, 12), scale=float(F32(2.0 / (n * PIX))))
    elif op == "dec_dgrad4":
        inp.update(dz4=_randn(rng, n * 576, 64, scale=gscale), a1=sp(f["a1"].astype(F32)), w4=K["w4"].reshape(32, 64))
    else:
        raise KeyError(op)
    return inp


# ---- the launch of one case through spdm_op_frame (include/spdm.h) ----------------------------------------------------------
def launch_plan(op, inp):
    """(dims, buffers, outputs): buffers ("in" | "inout", float32 array), ("out", elements) or None; outputs
    {name: (buffer index, shape)}.  d_sq and scale are the caller's (tests/test_gpu_frame_ops_fp64.py)."""
    I, O = (lambda a: ("in", np.ascontiguousarray(a, F32))), (lambda n: ("out", int(n)))
    IO = lambda a: ("inout", np.ascontiguousarray(a, F32))
    n = inp.get("n", 0)
    if op in ("enc_convs", "enc_kinks"):
        bufs = [I(inp[k]) for k in ("img", "w1", "b1", "w2", "b2", "w3", "b3")]
        if op == "enc_kinks":
            return [n], bufs + [IO(inp["feat"]), IO(inp["x3"])], {"feat": (7, (n, 9216)), "x3": (8, (n * 144, 128))}
        outs = {"feat": (7, (n, 9216))}
        if inp["train"]:
            outs["x3"] = (8, (n * 144, 128))
        return [n, inp["train"]], bufs + [O(n * 9216), O(n * 18432) if inp["train"] else None], outs
    if op == "enc_x2":
        return [n], [I(inp["img"]), I(inp["w1"]), I(inp["b1"]), O(n * 36864)], {"x2": (3, (n * 576, 64))}
    if op == "enc_dz3":
        return [n], [I(inp["dfeat"]), I(inp["feat"]), O(n * 9216)], {"dz3": (2, (n * 144, 64))}
    if op == "enc_dz2":
        return [n], [I(inp["dx3"]), I(inp["x3"]), O(n * 18432)], {"dz2": (2, (n * 144, 128))}
    if op == "enc_conv1_wgrad":
        return [n], [I(inp["img"]), I(inp["dx2"]), I(inp["x2"]), O(192), O(16)], {"dw": (3, (192,)), "db": (4, (16,))}
    if op == "add":
        return [n], [I(inp["src"]), IO(inp["dst"])], {"dst": (1, (n,))}
    if op == "dec_convs":
        tr = inp["train"]
        bufs = [I(inp[k]) for k in ("h0", "w2", "b2", "w4", "b4", "w6", "b6")] + [O(n * PIX)]
        bufs += [I(inp["target"]), O(n * 18432), O(n * 36864)] if tr else [None, None, None]
        outs = {"recon": (7, (n, 3, 96, 96))}
        if tr:
            outs.update(a1=(9, (n * 576, 32)), a2=(10, (n * 2304, 16)))
        return [n, tr], bufs, outs
    if op == "dec_kinks":
        bufs = [I(inp[k]) for k in ("latent", "w0", "b0", "w2", "b2", "w4", "b4")] + [IO(inp["a1"]), IO(inp["a2"])]
        return [n], bufs, {"a1": (7, (n * 576, 32)), "a2": (8, (n * 2304, 16))}
    if op == "dec_loss":
        return [n], [O(1)], {"loss": (0, (1,))}
    if op == "dec_bwd6":
        bufs = [I(inp[k]) for k in ("recon", "target", "a2", "w6")] + [O(n * 36864), O(192), O(3)]
        return [n], bufs, {"dz4": (4, (n * 2304, 16)), "dw": (5, (192,)), "db": (6, (3,))}
    if op == "dec_dgrad4":
        return [n], [I(inp["dz4"]), I(inp["a1"]), I(inp["w4"]), O(n * 18432)], {"dz2": (3, (n * 576, 32))}
    if op == "dec_colsum":
        M, C, fold = inp["M"], inp["C"], inp["fold"]
        return [M, C, fold], [I(inp["src"]), O(C // fold)], {"dst": (1, (C // fold,))}
    if op == "dec_unperm_conv":
        m = inp["cin"] * inp["cout"] * 4
        return [inp["cin"], inp["cout"]], [I(inp["src"]), O(m)], {"dst": (1, (m,))}
    if op == "dec_unperm_linear":
        return [], [I(inp["src"]), O(9216 * 128)], {"dst": (1, (9216 * 128,))}
    if op == "frame_wgrad":
        Co, Ci = FRAME_WG[inp["which"]][:2]
        return [inp["M"], inp["which"]], [I(inp["dy"]), I(inp["x"]), O(Co * Ci)], {"dst": (2, (Co, Ci))}
    raise KeyError(op)


def expected_info(op, inp):
    if op == "dec_colsum":
        return colsum_geometry(inp["M"])
    if op == "enc_conv1_wgrad":
        return (conv1_wgrad_blocks(inp["n"]),)
    if op == "frame_wgrad":
        return frame_wgrad_geometry(inp["M"], inp["which"]) + FRAME_WG[inp["which"]][:2]
    return None
