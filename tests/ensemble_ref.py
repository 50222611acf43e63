"""A numpy restatement of spdm_policy_select (csrc/policy.hip), written from its description in include/spdm.h alone: float64,
every operation an array operation of its own (numpy fuses nothing), every sum a Python loop in the stated order -- never
``np.sum``, whose pairwise order is another one.  The loops run over the summation index only; the environments, candidates and
pairs ride along as array axes, which changes no element's arithmetic.  Test support only."""
import numpy as np

MEDOID, COHERENT = 0, 1


def distances(x0, inp_h, cols):
    """``x0`` (E, K, H, D) float32 -> d (E, K, K) float64: d[e, j, k] = sum over r = inp_h .. H-1 (outer) and c < cols (inner) of
    ((double)x_j[r, c] - (double)x_k[r, c])^2, from 0.0; per term one subtraction, one multiplication, one addition."""
    assert x0.dtype == np.float32 and x0.ndim == 4
    E, K, H, D = x0.shape
    x = x0.astype(np.float64)
    d = np.zeros((E, K, K), dtype=np.float64)
    for r in range(inp_h, H):
        for c in range(cols):
            diff = x[:, :, None, r, c] - x[:, None, :, r, c]
            d = d + diff * diff
    return d


def medoid_scores(x0, inp_h, cols):
    """s (E, K): s_j = sum over k = 0 .. K-1, ascending, of d(j, k), from 0.0; d(j, j) is included."""
    d = distances(x0, inp_h, cols)
    s = np.zeros(d.shape[:2], dtype=np.float64)
    for k in range(d.shape[2]):
        s = s + d[:, :, k]
    return s


def coherent_scores(x0, guess, inp_h, rows, cols):
    """``guess`` (E, H, D) float32, one row per environment -> s (E, K): candidate j against the guess over rows
    [inp_h, inp_h + rows) and columns [0, cols), in the order of ``distances``."""
    assert x0.dtype == np.float32 and guess.dtype == np.float32 and guess.shape == (x0.shape[0],) + x0.shape[2:]
    assert 1 <= rows <= x0.shape[2] - inp_h
    x, g = x0.astype(np.float64), guess.astype(np.float64)
    s = np.zeros(x0.shape[:2], dtype=np.float64)
    for r in range(inp_h, inp_h + rows):
        for c in range(cols):
            diff = x[:, :, r, c] - g[:, None, r, c]
            s = s + diff * diff
    return s


def choose(scores):
    """(E, K) float64 -> (E) int32: the smallest j whose score is minimal; a NaN never wins against a number; all NaN: 0."""
    out = np.zeros(scores.shape[0], dtype=np.int32)
    for e, row in enumerate(scores):
        best = 0
        for j in range(1, row.shape[0]):
            if (np.isnan(row[best]) and not np.isnan(row[j])) or row[j] < row[best]:
                best = j
        out[e] = best
    return out


def U(n, tr, pos_min, pos_max):
    """The U of include/spdm.h: ``n`` float32 values, ``tr`` their float32 translations (broadcast), in float64."""
    assert n.dtype == np.float32 and tr.dtype == np.float32
    s = n.astype(np.float64) * 2.0 + tr.astype(np.float64)
    return (s + 1.0) / 2.0 * (np.float64(pos_max) - np.float64(pos_min)) + np.float64(pos_min)


def spread(x0, translation, pos_min, pos_max, inp_h):
    """(E, P) float64: the RMS distance, in the dataset's units, of the K candidates' way-point p from their mean."""
    assert x0.dtype == np.float32 and translation.dtype == np.float32
    E, K, H, D = x0.shape
    u = U(x0[:, :, inp_h:, 0], translation[:, None, None, 0], pos_min, pos_max)       # (E, K, P)
    v = U(x0[:, :, inp_h:, 1], translation[:, None, None, 1], pos_min, pos_max)
    su, sv = np.zeros((E, H - inp_h)), np.zeros((E, H - inp_h))
    for k in range(K):
        su = su + u[:, k]
        sv = sv + v[:, k]
    mu, mv = su / np.float64(K), sv / np.float64(K)
    q = np.zeros((E, H - inp_h))
    for k in range(K):
        du, dv = u[:, k] - mu, v[:, k] - mv
        q = q + (du * du + dv * dv)
    return np.sqrt(q / np.float64(K))


def select(x0, mode, inp_h, cols, guess=None, rows=0, translation=None, pos_min=None, pos_max=None):
    """``x0`` (E, K, H, D) float32 -> ``(chosen (E) int32, x0_out (E, H, D) float32, scores (E, K) float64, spread (E, P)
    float64 or None)``."""
    if mode == MEDOID:
        assert guess is None and rows == 0
        scores = medoid_scores(x0, inp_h, cols)
    else:
        assert mode == COHERENT
        scores = coherent_scores(x0, guess, inp_h, rows, cols)
    chosen = choose(scores)
    out = np.ascontiguousarray(x0[np.arange(x0.shape[0]), chosen])
    sp = spread(x0, translation, pos_min, pos_max, inp_h) if translation is not None else None
    return chosen, out, scores, sp
