"""The data and the torch restatement of a short autoencoder run for tests/test_gpu_autoencoder_fit.py.

``structured_frames``: uint8 frames a small autoencoder can learn something about in eight steps -- smooth gradients plus a
few flat rectangles, not white noise.  ``restate_run``: what ``train.fit`` does with ``autoencoder`` on them, in plain torch
on the host in a dtype of the caller's choice, from tests/autoencoder_ref.py's modules: the same initial weights, the same
batch order, MSELoss, clip of the global gradient norm at 0.5, Adam; then the mean over the validation frames of each
frame's mean squared error."""
import numpy as np
import torch

from autoencoder_ref import DEC_KEYS, decoder_forward_any
from encoder_train_ref import KEYS as ENC_KEYS
from encoder_train_ref import encoder_forward_any


def structured_frames(n: int = 40, seed: int = 5) -> np.ndarray:
    """(n, 96, 96, 3) uint8: per frame and channel a plane a + b x + c y over [0, 255], and three flat rectangles."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:96, 0:96].astype(np.float64) / 95.0
    img = np.empty((n, 96, 96, 3), np.uint8)
    for i in range(n):
        for c in range(3):
            a, b, d = rng.uniform(0.2, 0.8), rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)
            img[i, :, :, c] = np.clip(np.rint(255 * (a + b * (x - 0.5) + d * (y - 0.5))), 0, 255).astype(np.uint8)
        for _ in range(3):
            y0, x0 = rng.integers(0, 72, 2)
            h, w = rng.integers(8, 24, 2)
            img[i, y0:y0 + h, x0:x0 + w] = rng.integers(0, 256, 3, dtype=np.uint8)
    return img


def restate_run(state_dict, img_u8: np.ndarray, train_orders, val_ids, *, batch_size: int, lr: float = 1e-3, clip: float = 0.5,
                dtype=torch.float64):
    """``(val_loss before training, val_loss after it)`` as Python floats.  ``state_dict``: ``encoder.N.*`` / ``decoder.N.*``
    initial weights;  ``train_orders``: one array of store rows per epoch, in the order the loader yields them."""
    frames = (torch.from_numpy(img_u8).to(torch.float32) / 255).permute(0, 3, 1, 2).to(dtype)    # the store's float32(k) / 255
    enc = {k: state_dict["encoder." + k].detach().to(dtype).clone().requires_grad_(True) for k in ENC_KEYS}
    dec = {k: state_dict["decoder." + k].detach().to(dtype).clone().requires_grad_(True) for k in DEC_KEYS}
    params = list(enc.values()) + list(dec.values())
    opt = torch.optim.Adam(params, lr=lr)

    def val():
        with torch.no_grad():
            x = frames[torch.as_tensor(np.asarray(val_ids), dtype=torch.long)]
            return float(((decoder_forward_any(dec, encoder_forward_any(enc, x)) - x) ** 2).double().mean(dim=(1, 2, 3)).mean())

    first = val()
    for order in train_orders:
        order = np.asarray(order)
        for i in range(0, len(order), batch_size):
            x = frames[torch.as_tensor(order[i:i + batch_size], dtype=torch.long)]
            opt.zero_grad()
            loss = torch.mean((decoder_forward_any(dec, encoder_forward_any(enc, x)) - x) ** 2)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, clip)
            opt.step()
    return first, val()
