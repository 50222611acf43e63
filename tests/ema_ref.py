"""The EMA update of spdm_ema_step (csrc/optim.hip) restated in numpy float32, one rounding per operation:

    ema <- ema - omd * (ema - p),   omd = float32(1.0 - decay) with the subtraction in float64

which is the recipe ``s.sub_(one_minus_decay * (s - p))`` of diffusion-policy code bases.  tests/test_ema_reference.py holds it to
torch's own evaluation of that recipe on the CPU, bit for bit, and shows that the mutants below -- what a kernel that contracts,
reorders or swaps would compute -- differ from it on the data the GPU test uses; tests/test_gpu_ema.py holds the kernel to it."""
import numpy as np

SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1027, 4099)
DECAYS = (0.0, 0.405396, 0.9, 0.999, 0.9999)
KERNEL_DECAYS = (0.405396, 0.9)            # the decays at which every mutant differs (0.9999 alone hides the contracted form)


def omd_of(decay: float) -> np.float32:
    return np.float32(1.0 - float(decay))


def ema_step(ema: np.ndarray, p: np.ndarray, decay: float) -> np.ndarray:
    """One update; float32 in, float32 out, three individually rounded operations."""
    assert ema.dtype == np.float32 and p.dtype == np.float32 and ema.shape == p.shape
    omd = omd_of(decay)
    with np.errstate(all="ignore"):
        d = ema - p
        s = omd * d
        out = ema - s
    assert out.dtype == np.float32
    return out


def mutant_contracted(ema, p, decay):
    """fma(-omd, ema - p, ema): the product is not rounded (a float32 product is exact in float64; the sum is rounded there
    once more before float32, which moves a result in rare ties only)."""
    omd = omd_of(decay)
    d = ema - p
    return (ema.astype(np.float64) - np.float64(omd) * d.astype(np.float64)).astype(np.float32)


def mutant_convex(ema, p, decay):
    """d ema + (1 - d) p in float32."""
    return np.float32(decay) * ema + omd_of(decay) * p


def mutant_swapped(ema, p, decay):
    """the roles of ema and p exchanged"""
    return ema_step(p, ema, decay)


MUTANTS = {"contracted": mutant_contracted, "convex": mutant_convex, "swapped": mutant_swapped}


def make_pair(numel: int, seed: int = 0):
    """(ema, p): p ~ N(0, 1), ema = p + 1e-2 N(0, 1), float32."""
    rng = np.random.default_rng(1000 + 7 * numel + seed)
    p = rng.standard_normal(numel).astype(np.float32)
    ema = (p + np.float32(1e-2) * rng.standard_normal(numel).astype(np.float32)).astype(np.float32)
    return ema, p


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def one_ulp_bound(ema, p, out):
    """How far ``out = ema - 1 * (ema - p)`` may be from p: the two subtractions round once each (the product by 1 is exact),
    so half a unit of ema - p plus half a unit of the result.  For ema near p -- the shadow's case -- both units are at most
    p's and the sum is one ulp of p; an ema far above p rounds in its own, larger unit."""
    with np.errstate(all="ignore"):
        d = ema - p
    return 0.5 * np.spacing(np.abs(d)).astype(np.float64) + 0.5 * np.spacing(np.abs(out)).astype(np.float64)


def ema_decay(step, update_after_step=0, inv_gamma=1.0, power=0.75, min_value=0.0, max_value=0.9999):
    """optim.ema_decay restated (the warm-up schedule)."""
    n = max(0, step - update_after_step - 1)
    if n == 0:
        return 0.0
    return max(min_value, min(1.0 - (1.0 + n / inv_gamma) ** -power, max_value))
