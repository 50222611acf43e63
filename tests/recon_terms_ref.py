"""numpy restatement of spdm_recon_terms (csrc/train_metrics.hip, include/spdm.h) in the kernel's exact summation order, so
that the kernel's terms can be compared bit for bit: numpy's float64 arithmetic rounds every operation on its own, as the
kernel does.

Per frame of 27648 elements = 6912 quads of four consecutive floats (row-major): quad q belongs to partial q mod 256; a
partial starts at 0.0 and takes its quads in ascending order and within a quad the four elements in ascending order, as
``d = (double)target - (double)recon; p = p + d * d``; the 256 partials are combined by the tree ``for off in 128, 64, ..., 1:
p[i] = p[i] + p[i + off] (i < off)``; the term is ``p[0] / 27648.0``.

The keyword arguments are the knobs of tests/test_recon_terms_reference.py's mutants; their defaults are the contract."""
import numpy as np

FRAME = 3 * 96 * 96
PARTIALS = 256


def recon_terms(recon: np.ndarray, target: np.ndarray, *, partials: int = PARTIALS, acc=np.float64, divisor=None,
                drop_last_quad: bool = False, sign: float = -1.0) -> np.ndarray:
    """(n,) float64 terms of fp32 ``recon`` / ``target`` of shape (n, 3, 96, 96)."""
    assert recon.dtype == np.float32 and target.dtype == np.float32 and recon.shape == target.shape
    n = recon.shape[0]
    assert recon.reshape(n, -1).shape[1] == FRAME
    d = target.reshape(n, -1).astype(acc) + acc(sign) * recon.reshape(n, -1).astype(acc)      # t - r: the product by -1 is exact
    sq = (d * d).reshape(n, FRAME // 4 // partials, partials, 4)        # [round k][partial][element]: quad k * partials + partial
    if drop_last_quad:
        sq = sq.copy()
        sq[:, -1, -1, :] = 0
    p = np.zeros((n, partials), dtype=acc)
    for k in range(sq.shape[1]):
        for e in range(4):
            p = p + sq[:, k, :, e]
    off = partials // 2
    while off >= 1:
        p = p[:, :off] + p[:, off:2 * off]
        off //= 2
    return (p[:, 0] / acc(FRAME if divisor is None else divisor)).astype(np.float64)
