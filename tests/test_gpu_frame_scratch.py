"""The forward scratch of the two frame handles under a growing batch (csrc/spdm_api.hip FrameNet::grow).

``spdm_encoder_forward`` keeps the conv-3 maps of the chunk in flight in ``feat`` and ``spdm_decoder_forward`` the Linear's
output in ``h0``: [frames][9216] floats each, frames <= 2048.  A handle holds ONE such buffer, replaced when a call needs a
larger one.  A handle that kept every size it ever used would hold (512 + 768 + ... + 2048) x 9216 x 4 = 330 MB after the
calls below; one that replaces holds 2048 x 9216 x 4 = 75.5 MB, 66 MB more than after the 256-frame warm-up.

BOUND is twice the one buffer that may exist, which leaves room for the allocator's granularity.  It counts device memory
(``mem_get_info``), so torch's own allocations are kept out of the interval: the largest input and output exist before the
warm-up -- ``__call__`` allocates its result, which then comes out of the cached block of the largest one -- and results are
compared on the host.
"""
import pytest
import torch

from autoencoder_ref import make_decoder_state_dict
from oracle.encoder_ref import make_encoder_state_dict

pytestmark = pytest.mark.gpu

N_MAX = 2048                                   # frames of one chunk: the largest scratch a handle ever needs
BOUND = 2 * N_MAX * 9216 * 4


def _drop_under_growth(net, x, out_shape):
    """Free device memory lost between a 256-frame call and the same call after n = 512, 768, ..., 2048 on slices of x;
    the two 256-frame results must be equal."""
    dev = x.device
    room = torch.empty(N_MAX, *out_shape, device=dev)          # the largest result, once: later results reuse its block
    del room
    first = net(x[:256]).cpu()
    torch.cuda.synchronize(dev)
    free0 = torch.cuda.mem_get_info(dev)[0]
    for n in range(512, N_MAX + 1, 256):
        out = net(x[:n])
        assert tuple(out.shape) == (n, *out_shape)
        del out
    torch.cuda.synchronize(dev)
    free1 = torch.cuda.mem_get_info(dev)[0]
    assert torch.equal(net(x[:256]).cpu(), first)
    drop = free0 - free1
    print(f"{type(net).__name__}: free device memory fell by {drop} bytes ({drop / 2**20:.1f} MiB), bound {BOUND}")
    return drop


def test_encoder_forward_scratch_is_replaced():
    from state_policy_diffusionmodel_amd.vision import VisionEncoder
    enc = VisionEncoder(make_encoder_state_dict(5))
    g = torch.Generator(device=enc.device).manual_seed(31)
    x = torch.rand(N_MAX, 3, 96, 96, device=enc.device, generator=g)
    try:
        assert _drop_under_growth(enc, x, (128,)) < BOUND
    finally:
        enc.close()


def test_decoder_forward_scratch_is_replaced():
    from state_policy_diffusionmodel_amd.autoencoder import Decoder
    dec = Decoder(make_decoder_state_dict(6))
    g = torch.Generator(device=dec.device).manual_seed(32)
    z = 0.3 * torch.randn(N_MAX, 128, device=dec.device, generator=g)
    try:
        assert _drop_under_growth(dec, z, (3, 96, 96)) < BOUND
    finally:
        dec.close()
