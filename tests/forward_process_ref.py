"""numpy restatement of the training step's device random streams (include/spdm.h: spdm_train_forward_process)
on the oracle's Philox4x32-10.  Test infrastructure only.

Key = (seed lo, seed hi); counter = (q, sample, step, purpose) with sample = (uint32)(sample_offset + b).  Purpose 0 is the
sampler's stream (oracle.philox_ref.step_noise); 1 = noise, 2 = timestep, 3 = time-embedding dropout."""
from __future__ import annotations

import numpy as np

from oracle.philox_ref import _u01, normal_words, philox4x32_10

NOISE, TIMESTEP, DROPOUT = 1, 2, 3


def _key(seed: int):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def _samples(sample_offset: int, batch: int) -> np.ndarray:
    return np.array([(sample_offset + b) & 0xFFFFFFFF for b in range(batch)], dtype=np.uint32)


def draw_t(seed: int, step: int, sample_offset: int, batch: int, T: int) -> np.ndarray:
    """(batch,) int32 in [0, T): t_b = (w0 * T) >> 32."""
    w0 = philox4x32_10(np.uint32(0), _samples(sample_offset, batch), np.uint32(step), np.uint32(TIMESTEP), *_key(seed))[0]
    return ((w0.astype(np.uint64) * np.uint64(T)) >> np.uint64(32)).astype(np.int32)


def draw_noise(seed: int, step: int, sample_offset: int, batch: int, elems: int, purpose: int = NOISE) -> np.ndarray:
    """(batch, elems) fp32 normals: one Philox evaluation per four consecutive elements of a sample's window."""
    nq = (elems + 3) // 4
    q = np.arange(nq, dtype=np.uint32)[None, :]
    s = _samples(sample_offset, batch)[:, None]
    w = philox4x32_10(q, s, np.uint32(step), np.uint32(purpose), *_key(seed))
    z = np.stack(normal_words(*w), axis=-1).reshape(batch, nq * 4)
    return np.ascontiguousarray(z[:, :elems])


def keep_scale(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def draw_time_scale(seed: int, step: int, sample_offset: int, batch: int, time_dim: int, p: float) -> np.ndarray:
    """(batch, time_dim) fp32: keep ? 1 / (1 - p) : 0, keep iff u(word j & 3 of quad j >> 2) >= p in fp32."""
    nq = (time_dim + 3) // 4
    q = np.arange(nq, dtype=np.uint32)[None, :]
    s = _samples(sample_offset, batch)[:, None]
    w = philox4x32_10(q, s, np.uint32(step), np.uint32(DROPOUT), *_key(seed))
    u = np.stack([_u01(x) for x in w], axis=-1).reshape(batch, nq * 4)[:, :time_dim]
    return np.where(u >= np.float32(p), keep_scale(p), np.float32(0.0)).astype(np.float32)
