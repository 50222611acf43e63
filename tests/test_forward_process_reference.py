"""Properties of the training step's random streams on their numpy restatement, without a GPU."""
import numpy as np
import pytest

from forward_process_ref import DROPOUT, NOISE, TIMESTEP, draw_noise, draw_t, draw_time_scale, keep_scale
from oracle.philox_ref import step_noise

CASES = [(seed, step) for seed in (1234, 2024) for step in (0, 7)]


@pytest.mark.parametrize("seed,step", CASES)
def test_timesteps_cover_the_range_evenly(seed, step):
    t = draw_t(seed, step, 0, 4096, 16)
    counts = np.bincount(t, minlength=16)
    # expected 256 per value, sigma = sqrt(4096 * (1/16) * (15/16)) = 15.5: five sigma
    assert counts.size == 16 and counts.min() >= 178 and counts.max() <= 334, counts
    t = draw_t(seed, step, 0, 4096, 1000)
    assert t.dtype == np.int32 and t.min() >= 0 and t.max() <= 999
    assert t.min() < 10 and t.max() > 989            # 4096 draws: P(no draw in a 1 % tail) = 0.99^4096 ~ 1e-18


@pytest.mark.parametrize("seed,step", CASES)
def test_one_timestep_is_always_zero(seed, step):
    assert not draw_t(seed, step, 5, 64, 1).any()


@pytest.mark.parametrize("seed,step", CASES)
def test_noise_moments(seed, step):
    z = draw_noise(seed, step, 0, 512, 96)
    assert z.shape == (512, 96) and z.dtype == np.float32 and np.isfinite(z).all()
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02


@pytest.mark.parametrize("seed,step", CASES)
def test_dropout_keep_fraction_and_values(seed, step):
    m = draw_time_scale(seed, step, 0, 64, 256, 0.1)
    s = keep_scale(0.1)
    assert s == np.float32(1.0 / (1.0 - float(np.float32(0.1))))
    assert set(np.unique(m).tolist()) == {0.0, float(s)}
    assert abs(float((m != 0).mean()) - 0.9) < 0.01
    assert (draw_time_scale(seed, step, 0, 4, 10, 0.0) == 1.0).all()      # p = 0 keeps everything, unscaled


@pytest.mark.parametrize("seed,step", CASES)
def test_a_shard_draws_what_the_whole_batch_draws(seed, step):
    assert np.array_equal(draw_noise(seed, step, 3, 5, 115).view(np.uint32), draw_noise(seed, step, 0, 8, 115)[3:].view(np.uint32))
    assert np.array_equal(draw_t(seed, step, 3, 5, 1000), draw_t(seed, step, 0, 8, 1000)[3:])
    assert np.array_equal(draw_time_scale(seed, step, 3, 5, 10, 0.1), draw_time_scale(seed, step, 0, 8, 10, 0.1)[3:])


@pytest.mark.parametrize("seed,step", CASES)
def test_streams_are_mutually_different(seed, step):
    zs = {p: draw_noise(seed, step, 0, 8, 96, purpose=p) for p in (NOISE, TIMESTEP, DROPOUT)}
    zs[0] = step_noise(seed, step, 0, 8, 96)                              # the sampler's stream
    assert np.array_equal(zs[0], draw_noise(seed, step, 0, 8, 96, purpose=0))
    keys = sorted(zs)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert float(np.abs(zs[a] - zs[b]).max()) > 1.0, (a, b)       # independent normals: O(1) apart somewhere
            assert float(np.mean(zs[a] == zs[b])) < 0.01, (a, b)
    # a different step or seed is a different stream too
    assert float(np.abs(zs[NOISE] - draw_noise(seed, step + 1, 0, 8, 96)).max()) > 1.0
    assert float(np.abs(zs[NOISE] - draw_noise(seed + (1 << 32), step, 0, 8, 96)).max()) > 1.0


def test_the_sample_index_wraps_as_uint32():
    off = 2 ** 32 - 2
    z = draw_noise(1234, 0, off, 4, 48)
    assert np.array_equal(z[2:], draw_noise(1234, 0, 0, 2, 48))           # samples 2^32, 2^32 + 1 are samples 0, 1
    assert np.array_equal(z[:2], draw_noise(1234, 0, off, 2, 48))
    assert not np.array_equal(z[:2], z[2:])
    t = draw_t(1234, 0, off, 4, 1000)
    assert np.array_equal(t[2:], draw_t(1234, 0, 0, 2, 1000))
