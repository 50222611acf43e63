"""tests/sa_ref.py on the CPU: the float64 block reference equals the oracle's SelfAttention; the weight flavours make the
softmax as peaked as they claim; the fp32 CPU oracle meets sa_bound with the constants the GPU test uses; each model of a
kernel mistake exceeds it."""
import math

import pytest
import torch

from oracle.unet_film_ref import self_attention, unet_film_forward
from sa_ref import BLOCKS, COND, MUTANTS, flavour_weights, head_tile_samples, sa_block_ref, sa_bound, softmax_stats, worst_ratio

GEOMS = [(32, 3), (64, 6)]
_TAPS = {}


def taps64(flavour, H, D):
    """Block inputs from the float64 oracle: B = 4, t = 5 / 300 / 700 / 999, seed 1."""
    key = (flavour, H, D)
    if key not in _TAPS:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(4, 1, H, D, generator=g)
        y = torch.randn(4, 1, *COND, generator=g)
        sd64 = {k: v.double() for k, v in flavour_weights(flavour).items()}
        taps = {}
        unet_film_forward(sd64, x.double(), torch.tensor([5, 300, 700, 999]), y.double(), taps=taps)
        _TAPS[key] = {b: taps[i].float() for b, (i, _) in BLOCKS.items()}       # fp32-representable, as a device tap is
    return _TAPS[key]


def refs(flavour, H, D):
    sd = flavour_weights(flavour)
    return {b: sa_block_ref(sd, b, x) for b, x in taps64(flavour, H, D).items()}


@pytest.mark.parametrize("H,D", GEOMS)
def test_block_reference_equals_the_oracle(H, D):
    sd64 = {k: v.double() for k, v in flavour_weights("onehot").items()}
    for blk, x in taps64("onehot", H, D).items():
        got = sa_block_ref(sd64, blk, x)["out"]
        assert float((got - self_attention(sd64, blk, x.double())).abs().max()) <= 1e-12, blk


@pytest.mark.parametrize("H,D", GEOMS)
def test_flavours_are_as_peaked_as_they_claim(H, D):
    for blk, ref in refs("onehot", H, D).items():
        st = softmax_stats(ref)
        print(f"\nonehot {H} {blk}: range {st['range']:.0f} median max-p {st['median_max_p']:.2f}")
        assert st["median_max_p"] >= 0.4 and st["range"] >= 20, (blk, st["median_max_p"], st["range"])
    for blk, ref in refs("moderate", H, D).items():
        st = softmax_stats(ref)
        print(f"\nmoderate {H} {blk}: range {st['range']:.0f} median max-p {st['median_max_p']:.2f}")
        assert st["range"] >= 10 and st["median_max_p"] <= 0.85, (blk, st["median_max_p"], st["range"])
    # the longest block (L = 256 | 512): the key-block loop must move its running max
    st = softmax_stats(refs("onehot", H, D)["sa6"])
    rise8 = float((st["rise"] >= 8).double().mean())
    print(f"\nonehot {H} sa6: arg-max outside the first block {st['argmax_outside']:.2f}, rise >= 8 log2 units {rise8:.2f}")
    assert st["argmax_outside"] >= 0.25 and rise8 >= 0.05
    st = softmax_stats(refs("moderate", H, D)["sa6"])
    rise1 = float((st["rise"] >= 1).double().mean())
    print(f"\nmoderate {H} sa6: arg-max outside the first block {st['argmax_outside']:.2f}, rise >= 1 log2 unit {rise1:.2f}")
    assert st["argmax_outside"] >= 0.25 and rise1 >= 0.5


@pytest.mark.parametrize("flavour", ["plain", "moderate", "onehot", "onehot+widened"])
@pytest.mark.parametrize("H,D", GEOMS)
def test_fp32_oracle_meets_the_bound(H, D, flavour):
    sd = flavour_weights(flavour)
    for blk, ref in refs(flavour, H, D).items():
        r = worst_ratio(self_attention(sd, blk, taps64(flavour, H, D)[blk]), ref)
        print(f"\nfp32 oracle {flavour} {H} {blk}: error / bound {r:.3f}")
        assert r <= 1.0, (blk, r)


def _applies(mutant, c, n):
    if mutant == "skip_rescale":
        return n > 32                              # more than one 32-key block
    if mutant == "mask_finite":
        return head_tile_samples(c, n) > 1         # sa_head_kernel tiles that hold several samples
    return True


@pytest.mark.parametrize("H,D", GEOMS)
def test_every_mutant_exceeds_the_bound_on_onehot(H, D):
    """'mask_finite' as the issue words it -- the next sample's keys 30 logit units below the row max -- adds L exp(-30) ~ 1e-12
    of foreign v: below the rounding of fp32 itself, so no test of fp32 kernels can see it; asserted here is that arithmetic
    (error <= 2 L exp(-30) max |v| through the block) and that the same leak 10 units below the max (4.5e-5 per key) is
    rejected."""
    sd = flavour_weights("onehot")
    plain = flavour_weights("plain")
    for blk, x in taps64("onehot", H, D).items():
        ref = refs("onehot", H, D)[blk]
        c, n = x.shape[1], x.shape[2] * x.shape[3]
        ref1 = sa_block_ref(plain, blk, taps64("plain", H, D)[blk])
        for m in MUTANTS:
            if not _applies(m, c, n):
                continue
            gap = 10.0 if m == "mask_finite" else 30.0
            r = worst_ratio(sa_block_ref(sd, blk, x, mutant=m, gap=gap)["out"], ref)
            r1 = worst_ratio(sa_block_ref(plain, blk, taps64("plain", H, D)[blk], mutant=m, gap=gap)["out"], ref1)
            print(f"\nmutant {m} {H} {blk}: error / bound {r:.2f} on onehot, {r1:.2f} at g = 1")
            assert r > 1.0, (blk, m, r)
        if _applies("mask_finite", c, n):
            far = sa_block_ref(sd, blk, x, mutant="mask_finite", gap=30.0)["out"]
            err = float((far - ref["out"]).abs().max())
            assert err <= 2 * n * math.exp(-30.0) * float(ref["v"].abs().max()) * float((ref["A"] / ref["A"].clamp_max(1)).max()), err
            assert worst_ratio(far, ref) < 1e-3
