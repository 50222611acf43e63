"""The last SelfAttention block (sa6) computed only for the tokens outc reads (sa_fused.hip: sa_crop64_kernel), with and
without outc folded into its epilogue (SPDM_NO_SA_OUTC), against the full-token block (SPDM_NO_SA_CROP) and the oracle.
Geometries the cropped kernel does not take (H0 D > 128, or L > 256) run the full block either way and must agree too."""
import numpy as np
import pytest
import torch

from oracle.unet_film_ref import unet_film_forward
from state_policy_diffusionmodel_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
TOL = 1e-4
COND = (3, 11)
_SD = {}


def weights():
    if "sd" not in _SD:
        _SD["sd"] = random_state_dict(COND[0] * COND[1], seed=21)
    return _SD["sd"]


def make_engine(H, D, B, debug=False):
    from state_policy_diffusionmodel_amd.engine import SpdmEngine
    eng = SpdmEngine(H, D, COND[0] * COND[1], max_batch=B, debug=debug)
    eng.load_state_dict(weights())
    return eng


def inputs(H, D, B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, H, D, generator=g) * 1.5
    y = torch.randn(B, 1, *COND, generator=g)
    t = (torch.arange(B) * 37 + seed) % 1000
    return x, y, t


def run(eng, x, y, t, switches):
    for name in ("SPDM_NO_SA_CROP", "SPDM_NO_SA_OUTC", "SPDM_NO_FILM_FOLD", "SPDM_FILM_LOCAL"):
        eng.set_switch(name, name in switches)
    out = eng.unet_forward(x.cuda(), t, y.cuda()).cpu().numpy()
    assert not eng.nonfinite()
    return out


@pytest.mark.parametrize("H,D,batches", [(32, 3, (1, 3, 255, 256, 300)), (31, 5, (1, 3, 300)), (24, 4, (1, 3, 300)),
                                         (16, 3, (1, 3, 300)), (8, 1, (1, 3, 300)), (40, 2, (1, 3)), (64, 6, (1, 3))])
def test_cropped_block_matches_full_block_and_oracle(H, D, batches):
    Bmax = max(batches)
    x, y, t = inputs(H, D, Bmax, H * 100 + D)
    n_or = 3                                   # trajectories checked against the oracle (it is per trajectory)
    want = unet_film_forward(weights(), x[:n_or], t[:n_or], y[:n_or]).numpy()
    eng = make_engine(H, D, Bmax)
    try:
        for B in batches:
            xb, yb, tb = x[:B], y[:B], t[:B]
            for fold in ((), ("SPDM_NO_FILM_FOLD",), ("SPDM_FILM_LOCAL",)):
                full = run(eng, xb, yb, tb, fold + ("SPDM_NO_SA_CROP",))
                for extra in ((), ("SPDM_NO_SA_OUTC",)):
                    got = run(eng, xb, yb, tb, fold + extra)
                    assert np.abs(got - full).max() <= 2e-5, (H, D, B, fold, extra)
                    k = min(B, n_or)
                    assert np.abs(got[:k] - want[:k]).max() <= TOL, (H, D, B, fold, extra)
                assert np.abs(full[:min(B, n_or)] - want[:min(B, n_or)]).max() <= TOL, (H, D, B, fold)
    finally:
        eng.close()


@pytest.mark.parametrize("outc", [True, False])
def test_cropped_trajectory_is_bit_identical_alone_and_in_a_batch(outc):
    """One workgroup per trajectory: with the launch geometry pinned to the batch of 300 (SPDM_PIN_GEOMETRY, so the other
    launches reproduce a shard bit for bit), a trajectory run alone equals the same trajectory inside the batch."""
    H, D, B = 32, 3, 300
    x, y, t = inputs(H, D, B, 7)
    eng = make_engine(H, D, B)
    try:
        eng.set_switch("SPDM_PIN_GEOMETRY", True)
        sw = () if outc else ("SPDM_NO_SA_OUTC",)
        whole = run(eng, x, y, t, sw)
        for j in (0, 131, 299):
            alone = run(eng, x[j:j + 1], y[j:j + 1], t[j:j + 1], sw)
            assert np.array_equal(alone[0], whole[j]), j
    finally:
        eng.close()


def test_debug_engine_keeps_the_full_a6_tap():
    """Debug handles run the full-token block: the a6 tap is the whole (B, 64, Hp, Wp) map, equal to the oracle's."""
    H, D, B = 32, 3, 2
    x, y, t = inputs(H, D, B, 11)
    taps = {}
    want = unet_film_forward(weights(), x, t, y, taps=taps).numpy()
    eng = make_engine(H, D, B, debug=True)
    try:
        got = eng.unet_forward(x.cuda(), t, y.cuda()).cpu().numpy()
        a6 = eng.debug_tensor("a6").cpu().numpy()
    finally:
        eng.close()
    assert np.abs(got - want).max() <= TOL
    assert a6.shape == tuple(taps["a6"].shape)
    assert np.abs(a6 - taps["a6"].numpy()).max() <= TOL
