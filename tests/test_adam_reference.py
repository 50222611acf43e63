"""tests/adam_ref.py (the float64 numpy statement of clip + Adam that the GPU tests measure against) pinned to
``torch.optim.Adam`` + ``torch.nn.utils.clip_grad_norm_`` run in float64 on the CPU: 5 steps, with and without clipping, with a
mid-run learning-rate change, to 1e-12 relative."""
import numpy as np
import pytest
import torch

from adam_ref import RefAdam, clip_coef, grad_norm, make_inputs

SIZES = [(1,), (3,), (1025,), (4, 1023, 7001)]


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("max_norm", [None, 0.5, 1e6])
def test_reference_equals_torch_float64(sizes, max_norm):
    params, grads = make_inputs(sizes, steps=5)
    ref = RefAdam(params)
    tp = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p in params]
    opt = torch.optim.Adam(tp, lr=1e-3)
    lr = 1e-3
    for i, gs in enumerate(grads):
        if i == 3:                    # halved before step 4, through param_groups as a scheduler would
            lr *= 0.5
            opt.param_groups[0]["lr"] = lr
        for p, g in zip(tp, gs):
            p.grad = torch.from_numpy(g.astype(np.float64))
        want_norm = None
        if max_norm:
            want_norm = float(torch.nn.utils.clip_grad_norm_(tp, max_norm))
        opt.step()
        norm = ref.step(gs, lr, max_norm)
        if want_norm is not None:
            assert abs(norm - want_norm) <= 1e-12 * want_norm
    for k, p in enumerate(tp):
        st = opt.state[p]
        for name, got, want in (("p", ref.p[k], p.detach().numpy()), ("exp_avg", ref.m[k], st["exp_avg"].numpy()),
                                ("exp_avg_sq", ref.v[k], st["exp_avg_sq"].numpy())):
            scale = float(np.max(np.abs(want)))
            assert float(np.max(np.abs(got - want))) <= 1e-12 * scale, (name, k)
        assert int(st["step"]) == ref.t == 5


def test_clip_semantics():
    g = [np.array([3.0, 0.0]), np.array([4.0])]
    assert grad_norm(g) == 5.0                                     # one norm over all segments
    assert clip_coef(5.0, 0.5) == 0.5 / (5.0 + 1e-6)
    assert clip_coef(0.25, 0.5) == 1.0                             # below max_norm: untouched
    assert clip_coef(5.0, None) == 1.0 and clip_coef(5.0, 0) == 1.0
    assert np.isnan(clip_coef(float("nan"), 0.5))                  # propagates, as clip_grad_norm_'s does
    assert clip_coef(float("inf"), 0.5) == 0.0


def test_gradients_are_only_read():
    params, grads = make_inputs((37,), steps=1)
    before = grads[0][0].copy()
    RefAdam(params).step(grads[0], 1e-3, 0.5)
    assert np.array_equal(before, grads[0][0])
