"""tests/level3_chain_ref.py (the float64 restatement tests/test_gpu_conv_chain.py checks conv_chain.hip against) against the
oracle's DoubleConvolution on a width-1 map, where only the centre column of a 3 x 3 kernel sees data."""
import numpy as np
import torch

import level3_chain_ref as R
from oracle.unet_film_ref import double_conv


def _w9(w):
    t = torch.zeros(w.shape[1], w.shape[2], 3, 3, dtype=torch.float64)
    t[:, :, :, 1] = torch.from_numpy(w).permute(1, 2, 0)
    return t


def test_two_layer_chain_is_the_oracles_double_convolution():
    g = np.random.default_rng(0)
    for B, HW, C in ((3, 4, 64), (2, 8, 128)):
        x = g.standard_normal((B, HW, C))
        w1, w2 = g.standard_normal((3, C, C)) * 0.1, g.standard_normal((3, C, C)) * 0.1
        gm, bt = g.uniform(-1.5, 1.5, C), g.uniform(-0.5, 0.5, C)
        raw = R.chain(x, [w1, w2], [None, gm], [None, bt], [0, 1])
        got = R.group_norm(raw[-1], gm, bt)
        sd = {"p.first.weight": _w9(w1), "p.second.weight": _w9(w2), "p.norm.weight": torch.from_numpy(gm), "p.norm.bias": torch.from_numpy(bt)}
        xn = torch.from_numpy(x).reshape(B, HW, 1, C).permute(0, 3, 1, 2)
        want = double_conv(sd, "p", xn).permute(0, 2, 3, 1).reshape(B, HW, C).numpy()
        assert np.abs(got - want).max() <= 1e-12
        s = R.sums(raw[-1])
        assert np.allclose(s[:, 0], raw[-1].reshape(B, -1).sum(1)) and np.allclose(s[:, 1], (raw[-1] ** 2).reshape(B, -1).sum(1))


def test_no_tap_leaves_a_sample():
    g = np.random.default_rng(1)
    x = g.standard_normal((2, 4, 64))
    w = [g.standard_normal((3, 64, 64))]
    a = R.chain(x, w, [None], [None], [0])[-1]
    x2 = x.copy()
    x2[1] *= 100.0
    b = R.chain(x2, w, [None], [None], [0])[-1]
    assert (a[0] == b[0]).all() and not (a[1] == b[1]).all()
