"""tests/ema_ref.py against torch on the CPU, its mutants against it, and optim.ema_decay's schedule (no GPU).

The restatement is the reference of tests/test_gpu_ema.py's bit comparisons, so it is held to torch's own evaluation of the
recipe first, and the forms a wrong kernel would compute are shown to differ from it on that test's data: a bit-equality test
against a reference that no mutant can be told from proves nothing."""
import numpy as np
import pytest
import torch

import ema_ref
from state_policy_diffusionmodel_amd.optim import EMA_SCHEDULE, ema_decay


@pytest.mark.parametrize("decay", ema_ref.DECAYS)
@pytest.mark.parametrize("numel", ema_ref.SIZES)
def test_restatement_equals_torchs_sub_recipe_bit_for_bit(numel, decay):
    ema, p = ema_ref.make_pair(numel)
    e, q = torch.from_numpy(ema.copy()), torch.from_numpy(p.copy())
    e.sub_((e - q) * (1.0 - decay))
    want = ema_ref.ema_step(ema, p, decay)
    assert np.array_equal(ema_ref.bits(e.numpy()), ema_ref.bits(want))
    assert np.array_equal(q.numpy(), p)


def test_lerp_is_another_function():
    """torch.lerp_ is not the recipe: over the same grid it differs somewhere (the reason the kernel does not restate it)."""
    differing = 0
    for numel in ema_ref.SIZES:
        for decay in ema_ref.DECAYS:
            ema, p = ema_ref.make_pair(numel)
            e = torch.from_numpy(ema.copy())
            e.lerp_(torch.from_numpy(p.copy()), 1.0 - decay)
            differing += int((ema_ref.bits(e.numpy()) != ema_ref.bits(ema_ref.ema_step(ema, p, decay))).sum())
    print(f"\nEMA lerp_ vs the sub_ recipe: {differing} differing elements")
    assert differing > 0


@pytest.mark.parametrize("decay", ema_ref.KERNEL_DECAYS)
@pytest.mark.parametrize("name", sorted(ema_ref.MUTANTS))
def test_mutants_differ_on_the_gpu_tests_data(name, decay):
    ema, p = ema_ref.make_pair(4099)
    want = ema_ref.ema_step(ema, p, decay)
    got = ema_ref.MUTANTS[name](ema, p, decay)
    count = int((ema_ref.bits(got) != ema_ref.bits(want)).sum())
    print(f"\nEMA mutant {name} at decay {decay}: {count} of 4099 elements differ")
    assert count > 0
    if name == "swapped":
        assert count == 4099
    if name == "convex":
        assert count > 1000


def test_the_contracted_mutant_hides_at_0_9999():
    """Why 0.9999 alone is not a test point: there the contracted form equals the restatement on this data."""
    ema, p = ema_ref.make_pair(4099)
    assert np.array_equal(ema_ref.bits(ema_ref.mutant_contracted(ema, p, 0.9999)), ema_ref.bits(ema_ref.ema_step(ema, p, 0.9999)))


def test_edge_values():
    ema, p = ema_ref.make_pair(257)
    assert np.array_equal(ema_ref.bits(ema_ref.ema_step(ema, p, 1.0)), ema_ref.bits(ema))          # omd = 0: unchanged
    first = ema_ref.ema_step(ema, p, 0.0)                                                          # omd = 1: one ulp from p
    assert np.all(np.abs(first.astype(np.float64) - p) <= ema_ref.one_ulp_bound(ema, p, first))
    near = np.abs(p) >= 0.1                     # ema within 0.06 of such a p: both roundings are in p's unit or below
    assert near.sum() > 200 and np.all(np.abs(first.astype(np.float64) - p)[near] <= np.spacing(np.abs(p))[near])
    q = p.copy()
    q[3], q[100] = np.nan, np.inf
    out = ema_ref.ema_step(ema, q, 0.9)
    assert np.isnan(out[3]) and np.isinf(out[100]) and np.isfinite(np.delete(out, [3, 100])).all()


PINNED = {1: 0.0, 2: 0.405396, 3: 0.561309, 10: 0.822172, 100: 0.968377, 1000: 0.994377, 10000: 0.999, 100000: 0.999822,
          1000000: 0.9999}


def test_schedule_values():
    for step, want in PINNED.items():
        assert round(ema_decay(step), 6) == want, step
        assert ema_decay(step) == ema_ref.ema_decay(step)
    assert ema_decay(0) == 0.0 and isinstance(ema_decay(5), float)
    assert EMA_SCHEDULE == dict(update_after_step=0, inv_gamma=1.0, power=0.75, min_value=0.0, max_value=0.9999)


def test_schedule_is_monotone_clamps_and_waits():
    values = [ema_decay(s) for s in range(0, 3000)] + [ema_decay(10 ** k) for k in range(4, 10)]
    assert all(b >= a for a, b in zip(values, values[1:]))
    assert max(values) == 0.9999 and ema_decay(10 ** 9) == 0.9999                  # max_value
    assert ema_decay(10 ** 9, max_value=0.99) == 0.99 and ema_decay(50, max_value=0.5) == 0.5
    assert ema_decay(2, min_value=0.6) == 0.6 and ema_decay(1, min_value=0.6) == 0.0       # the first update copies whatever min is
    assert [ema_decay(s, update_after_step=10) for s in (1, 10, 11)] == [0.0, 0.0, 0.0]
    assert ema_decay(12, update_after_step=10) == ema_decay(2) and ema_decay(110, update_after_step=10) == ema_decay(100)
    assert ema_decay(11, inv_gamma=10.0) == ema_decay(2) and ema_decay(3, power=1.0) == pytest.approx(2.0 / 3.0)
