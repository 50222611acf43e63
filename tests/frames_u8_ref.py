"""numpy restatement of spdm_frames_to_bytes (csrc/dataset.hip, include/spdm.h): planar fp32 frames to interleaved uint8 pixels,
each frame one 96 x 96 tile of a contact sheet.

Quantisation in fp32: ``v = x * 255.0f`` (one fp32 multiply), ``q = rint(v)`` (ties to even), the byte is 0 if v is NaN, else
``clamp(q, 0, 255)``.  Frame i is tile ``j = tile_offset + i`` at tile row ``j // cols`` and tile column ``j % cols``: pixel
``(y, x, c)`` lands at ``out[(j // cols) * 96 + y, (j % cols) * 96 + x, c]``; other tiles keep what ``out`` held.

The keyword arguments after ``out`` are the knobs of tests/test_frames_u8_reference.py's mutants; their defaults are the
contract."""
import numpy as np


def quantise(x: np.ndarray, *, mul=np.float32, floor_half: bool = False) -> np.ndarray:
    assert x.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        v = x.astype(mul) * mul(255.0)
        q = np.floor(v + mul(0.5)) if floor_half else np.rint(v)
        q = np.where(np.isnan(v), mul(0.0), np.clip(q, mul(0.0), mul(255.0)))
    return q.astype(np.uint8)


def edge_values() -> np.ndarray:
    """The values at which a quantiser goes wrong: all 256 ``float32(k) / 255``; around the ties ``(k + 0.5) / 255`` for k in
    {0, 1, 127, 254} the 16 float32 neighbours on each side (and the value itself); -0.0, negatives, values above 1, the
    infinities and NaN."""
    vals = [np.arange(256, dtype=np.float32) / np.float32(255)]
    for k in (0, 1, 127, 254):
        mid = np.float32((k + 0.5) / 255)
        bits = mid.view(np.int32) + np.arange(-16, 17, dtype=np.int32)
        vals.append(bits.view(np.float32))
    vals.append(np.array([-0.0, -1e-9, -0.3, -1.0, -1e30, 1.0000001, 1.002, 1.5, 300.0, 1e30, np.inf, -np.inf, np.nan], np.float32))
    return np.concatenate(vals)


def edge_frames(n: int, seed: int = 0) -> np.ndarray:
    """(n, 3, 96, 96) fp32: uniform values over [-0.1, 1.1) with ``edge_values()`` scattered over every frame at seeded places"""
    rng = np.random.default_rng(seed)
    x = (rng.random((n, 3 * 96 * 96), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
    edge = edge_values()
    for i in range(n):
        x[i, rng.choice(x.shape[1], edge.size, replace=False)] = edge
    return x.reshape(n, 3, 96, 96)


def sheet_shape(n_tiles: int, cols: int):
    return (-(-n_tiles // cols) * 96, cols * 96, 3)


def frames_to_u8(frames: np.ndarray, cols: int = 1, tile_offset: int = 0, n_tiles=None, out=None, *, mul=np.float32,
                 floor_half: bool = False, swap_xy: bool = False, reverse_channels: bool = False, swap_tile: bool = False):
    """``frames`` (n, 3, 96, 96) fp32 -> the sheet (a copy of ``out``, or zeros), uint8 ``sheet_shape(n_tiles, cols)``."""
    n = frames.shape[0]
    n_tiles = tile_offset + n if n_tiles is None else n_tiles
    assert frames.shape[1:] == (3, 96, 96) and cols >= 1 and 0 <= tile_offset and tile_offset + n <= n_tiles
    sheet = np.zeros(sheet_shape(n_tiles, cols), np.uint8) if out is None else out.copy()
    assert sheet.shape == sheet_shape(n_tiles, cols)
    pix = quantise(frames, mul=mul, floor_half=floor_half).transpose(0, 3, 2, 1) if swap_xy else \
        quantise(frames, mul=mul, floor_half=floor_half).transpose(0, 2, 3, 1)                   # (n, y, x, c)
    if reverse_channels:
        pix = pix[..., ::-1]
    for i in range(n):
        j = tile_offset + i
        r, c = (j % cols, j // cols) if swap_tile else (j // cols, j % cols)
        if r * 96 < sheet.shape[0] and c < cols:
            sheet[r * 96:(r + 1) * 96, c * 96:(c + 1) * 96] = pix[i]
    return sheet
