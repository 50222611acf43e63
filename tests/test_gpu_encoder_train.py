"""The observation encoder's training pass on the HIP path (spdm_encoder_train_forward / _backward / _update_weights,
vision.VisionEncoder) against float64 autograd through tests/encoder_train_ref.py.

Bound: per tensor ||g - g64||_2 <= 1e-4 ||g64||_2, the project's training bound (tests/test_gpu_train_grad.py::BOUND).
grad_latent is random at the scale 1 / (n 128); frames are U[0,1) with a zero corner patch and a last row of ones.  The
float64 reference picks its own ReLU masks.

The fp32 forward rounds a pre-activation within ~1e-7 of zero to either side of its ReLU kink; on the n = 2100 frames 2 of
the 38,707,200 conv-2 units do, and with the fp32 masks that alone moved 0.weight / 0.bias / 2.weight / 2.bias by 4.2e-4 /
4.4e-4 / 3.0e-4 / 3.0e-4 (torch-CPU fp32 autograd misses float64 by 3.9e-4 / 4.1e-4 / 3.1e-4 / 3.0e-4 on the same input).
The training forward therefore settles the saved maps' signs by a float64 evaluation (encoder_kinks_kernel).

Measured (MI355X), worst ratio per tensor over n = 1, 6, 40, 2100: 0.weight 3.2e-7, 0.bias 4.3e-7, 2.weight 9.4e-7,
2.bias 6.8e-7, 4.weight 6.6e-7, 4.bias 6.2e-7, 7.weight 3.3e-7, 7.bias 8.4e-8; n = 2100 against the sum of 128-frame runs
<= 1.1e-6; border case <= 5.4e-7; after update_weights <= 2.7e-7.  The ("trained", n) cases (convolutions scaled by 3, dead
channels, 8-bit frames with a black band on the padded border and flat patches): <= 5.0e-7.
"""
import ctypes

import pytest
import torch

from autoencoder_ref import case_id, trained_encoder_state_dict, trained_frames
from encoder_train_ref import KEYS, encoder_forward_any, encoder_grads, images
from oracle.encoder_ref import encoder_forward, make_encoder_state_dict

pytestmark = pytest.mark.gpu

BOUND = 1e-4
TOL = 1e-4


def _encoder(seed=5):
    from state_policy_diffusionmodel_amd.vision import VisionEncoder
    sd = make_encoder_state_dict(seed)
    return sd, VisionEncoder(sd)


def _grad_latent(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 128, generator=g) / (n * 128)


def _ratios(got, want):
    out = {}
    for k in KEYS:
        g, w = got[k].detach().double().cpu(), want[k].double()
        assert g.shape == w.shape, k
        out[k] = float((g - w).norm() / w.norm())
    return out


def _assert_within(tag, worst):
    print(f"\nENCODER GRAD {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= BOUND}
    assert not bad, "||g - g64|| / ||g64|| above %g: %s" % (BOUND, ", ".join(f"{k} {v:.2e}" for k, v in sorted(bad.items())))


@pytest.mark.parametrize("n", [1, 7, 2100])
def test_train_forward_equals_forward_bit_for_bit(n):
    """n = 2100 crosses the 2048-frame chunk."""
    sd, enc = _encoder()
    try:
        x = images(n, n).cuda()
        assert torch.equal(enc.train_forward(x), enc(x))
    finally:
        enc.close()


@pytest.mark.parametrize("n", [1, 6, 40, 2100, ("trained", 6), ("trained", 40)], ids=case_id)
def test_gradients_match_float64_autograd(n):
    """The ("trained", n) cases: convolutions scaled by 3 with dead channels, 8-bit frames with a black band on the padded border
    and flat patches."""
    from state_policy_diffusionmodel_amd.vision import VisionEncoder
    tag = case_id(n)
    if isinstance(n, int):
        sd, x = make_encoder_state_dict(5), images(n, 100 + n)
    else:
        n = n[1]
        sd, x = trained_encoder_state_dict(make_encoder_state_dict(5)), trained_frames(n, 100 + n)
    enc = VisionEncoder(sd)
    try:
        gl = _grad_latent(n, n)
        lat64, g64 = encoder_grads(sd, x, gl)
        lat = enc.train_forward(x.cuda())
        assert float((lat.cpu().double() - lat64).abs().max()) <= TOL
        flat = enc.backward(gl.cuda())
        torch.cuda.synchronize()
        grads = enc.grads()
        assert set(grads) == set(KEYS)
        assert all(grads[k].data_ptr() >= flat.data_ptr() for k in KEYS)          # views of the flat gradient
        _assert_within(f"n={tag}", _ratios(grads, g64))
    finally:
        enc.close()


def test_large_n_equals_the_sum_of_small_runs():
    """n = 2100 (two chunks, the second accumulated onto the first) against the sum of this encoder's own runs on
    128-frame pieces, which the small-n cases above tie to float64.  The two differ in fp32 summation order only; the bound
    is the training bound."""
    sd, enc = _encoder()
    try:
        n = 2100
        x, gl = images(n, 100 + n).cuda(), _grad_latent(n, n).cuda()
        enc.train_forward(x)
        enc.backward(gl)
        full = {k: v.double().clone() for k, v in enc.grads().items()}
        acc = {k: torch.zeros_like(v) for k, v in full.items()}
        for i in range(0, n, 128):
            enc.train_forward(x[i:i + 128].contiguous())
            enc.backward(gl[i:i + 128].contiguous())
            for k, v in enc.grads().items():
                acc[k] += v.double()
        _assert_within("n=2100 vs pieces", _ratios(full, {k: v.cpu() for k, v in acc.items()}))
    finally:
        enc.close()


def test_conv1_border_windows():
    """0.weight / 0.bias when only the border of conv 1's map receives gradient: the windows that read the zero padding
    (row / column 0) and the last ones conv 2 reads (row / column 47).  grad_latent reaches conv 1 through
    Linear(9216,128), whose 128 inputs cannot single out map positions for generic weights (6400 interior constraints on
    128 unknowns), so the case is set up on the Linear instead: 7.weight is zero for every interior conv-3 position, and
    any grad_latent then puts gradient on conv-3 rows / columns 0 and 11 only, i.e. conv-1 rows / columns 0..3 and
    44..47.  Frames and grad_latent are the generic ones."""
    from state_policy_diffusionmodel_amd.vision import VisionEncoder
    sd = make_encoder_state_dict(8)
    sd["7.weight"].view(128, 64, 12, 12)[:, :, 1:11, 1:11] = 0.0
    enc = VisionEncoder(sd)
    try:
        n = 6
        x, gl = images(n, 3), _grad_latent(n, 9)
        _, g64 = encoder_grads(sd, x, gl)
        assert float(g64["0.weight"].norm()) > 0.0
        enc.train_forward(x.cuda())
        enc.backward(gl.cuda())
        r = _ratios(enc.grads(), g64)
        _assert_within("border", {k: r[k] for k in ("0.weight", "0.bias", "2.weight", "4.weight")})
    finally:
        enc.close()


def test_determinism_and_call_order():
    from state_policy_diffusionmodel_amd import _lib
    sd, enc = _encoder()
    try:
        n = 40
        x, gl = images(n, 1).cuda(), _grad_latent(n, 2).cuda()
        with pytest.raises(RuntimeError, match=r"\(-3\)"):                 # SPDM_ERR_STATE: no forward yet
            enc.backward(gl)
        enc.train_forward(x)
        a = enc.backward(gl).clone()
        with pytest.raises(RuntimeError, match=r"\(-3\)"):                 # one backward per forward
            enc.backward(gl)
        enc.train_forward(x)
        b = enc.backward(gl).clone()
        assert torch.equal(a, b)
        enc.train_forward(x)
        enc.update_weights(enc.flat_parameter().detach())
        rc = enc.lib.spdm_encoder_backward(enc._h, n, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(gl.data_ptr()),
                                           ctypes.c_void_p(a.data_ptr()), None)
        assert rc == _lib.SPDM_ERR_STATE                                   # an update in between invalidates the forward
        enc.train_forward(x)
        rc = enc.lib.spdm_encoder_backward(enc._h, n - 1, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(gl.data_ptr()),
                                           ctypes.c_void_p(a.data_ptr()), None)
        assert rc == _lib.SPDM_ERR_STATE                                   # another n_images
    finally:
        enc.close()


def test_update_weights_equals_a_fresh_handle():
    from state_policy_diffusionmodel_amd.vision import VisionEncoder
    from state_policy_diffusionmodel_amd.weights import pack_state_dict
    sd, enc = _encoder(5)
    new = make_encoder_state_dict(6)
    fresh = VisionEncoder(new)
    try:
        x = images(7, 4).cuda()
        enc.train_forward(x)                                               # a training handle: the transposed copies follow too
        blob, _ = pack_state_dict({k: new[k] for k in KEYS})
        enc.update_weights(torch.from_numpy(blob).cuda())
        got = enc(x)
        assert torch.equal(got, fresh(x))
        assert float((got.cpu() - encoder_forward(new, x.cpu())).abs().max()) <= TOL
        assert all(torch.equal(enc.state_dict()[k], new[k]) for k in KEYS)
        gl = _grad_latent(7, 1)
        _, g64 = encoder_grads(new, x.cpu(), gl)
        enc.train_forward(x)
        enc.backward(gl.cuda())
        _assert_within("after update", _ratios(enc.grads(), g64))
    finally:
        enc.close()
        fresh.close()
