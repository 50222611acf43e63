"""The dataset on the device: windows, statistics and normalisation of the reference's ``CarRacingDataset``, with the frames
kept in HBM and every training batch assembled by ONE HIP launch (``spdm_dataset_gather``).

Replaces utils/load_data.py:11-182 and utils/data_utils.py:10-62: ``create_sample_indices_sparse``, ``_compute_stats``,
``normalize_data`` / ``_normalize_position``, ``__getitem__`` under a 4-worker ``DataLoader``, and the host-to-device copy of
every batch.  A batch is a list of window numbers; ``DeviceDataset.batch`` turns it into the dict of float32 device tensors
that ``Diffusion_DDPM.training_step`` takes, bit for bit what the reference's numpy float64 arithmetic gives after the
model's ``.float()``.

Frames are stored as uint8 where that is exact.  The data generators write ``img / 255.0``, so every stored value is
``k / 255.0`` for a byte ``k``, and ``float32(k) / float32(255)`` equals ``float32(k / 255.0)`` for all 256 bytes
(tests/test_dataset_reference.py); a store with any other value is kept as float32.

Reading zarr is not part of this module's tested surface (zarr is an optional import of ``CarRacingDataModule.setup``); the
arrays are passed in as numpy arrays.  There is no CPU fallback: ``batch`` and ``frames`` need the GPU."""
from __future__ import annotations

import ctypes
import os
import pickle
from typing import Optional

import numpy as np
import torch

from . import _lib
from .weights import normalize_data, unnormalize_data, unnormalize_position  # noqa: F401  (re-exported: the reference's formulas, written once)

FRAME_SHAPE = (96, 96, 3)
_CHUNK_ROWS = 256        # frames per piece of the uint8 check and of the upload: 28 MB of float32


# ---- numpy helpers (utils/data_utils.py:46-56, utils/load_data.py:58-78) ------------------------------------------------------
def create_sample_indices_sparse(ends, sequence_length: int, step_size: int) -> np.ndarray:
    """``(N, 4)`` int64 rows ``[start, start + sequence_length * step_size, 0, sequence_length]``: for each episode
    ``[prev_end, end)`` every ``start`` in ``[prev_end, end - sequence_length]`` whose strided window still ends inside the
    episode, ``start + sequence_length * step_size <= end``."""
    rows = []
    prev_end = 0
    for end in np.asarray(ends).reshape(-1).tolist():
        end = int(end)
        starts = np.arange(prev_end, end - sequence_length + 1, dtype=np.int64)
        starts = starts[starts + sequence_length * step_size <= end]
        rows.append(np.stack([starts, starts + sequence_length * step_size, np.zeros_like(starts),
                              np.full_like(starts, sequence_length)], axis=1))
        prev_end = end
    return np.concatenate(rows, axis=0) if rows else np.zeros((0, 4), np.int64)


def _min_max(data):
    data = data.reshape(-1, data.shape[-1])
    return {"min": np.min(data, axis=0), "max": np.max(data, axis=0)}


def compute_stats(position, velocity, action, indices, step_size: int) -> dict:
    """The reference's statistics dict.  Position ``min`` / ``max`` are SCALARS: the average, over all windows and both
    columns, of each window's per-column minimum (maximum).  Velocity and action: per-column min / max of the whole array."""
    indices = np.asarray(indices)
    seq = int(indices[0, 3]) if len(indices) else 0
    rows = indices[:, 0:1] + step_size * np.arange(seq)[None, :]            # (N, seq): the rows of data[start:end:step]
    win = np.asarray(position)[rows]                                          # (N, seq, 2)
    pos = {"max": np.average(win.max(axis=1)), "min": np.average(win.min(axis=1))}
    return {"position": pos, "velocity": _min_max(np.asarray(velocity)), "action": _min_max(np.asarray(action))}


def split_indices(n: int, seed=None):
    """``random_split(range(n), [int(0.8 n), n - int(0.8 n)], generator)``'s two index lists: the head and the tail of one
    ``torch.randperm(n)``; ``seed`` falsy means torch's default generator, as in the reference."""
    g = torch.Generator().manual_seed(seed) if seed else torch.default_generator
    perm = torch.randperm(n, generator=g).numpy()
    n_train = int(n * 0.8)
    return perm[:n_train], perm[n_train:]


# ---- image storage ------------------------------------------------------------------------------------------------------------
def _fits_uint8(chunk: np.ndarray) -> bool:
    with np.errstate(invalid="ignore"):
        k = np.rint(chunk * 255)
        ok = (k >= 0) & (k <= 255) & (k.astype(np.float32) / np.float32(255) == chunk.astype(np.float32))
    return bool(ok.all())


def choose_image_storage(img: np.ndarray, image_storage: str = "auto", chunk_rows: int = _CHUNK_ROWS) -> str:
    """``'uint8'`` or ``'float32'``.  uint8 is exact iff every value ``v`` satisfies
    ``float32(rint(v * 255)) / float32(255) == float32(v)`` (checked ``chunk_rows`` frames at a time); ``'auto'`` takes it
    then, ``'uint8'`` insists on it (ValueError otherwise), ``'float32'`` never looks.  A uint8 array is raw pixels."""
    if image_storage not in ("auto", "uint8", "float32"):
        raise ValueError(f"image_storage must be 'auto', 'uint8' or 'float32', got {image_storage!r}")
    if img.dtype == np.uint8:
        if image_storage == "float32":
            raise ValueError("a uint8 image array is stored as uint8")
        return "uint8"
    if image_storage == "float32":
        return "float32"
    fits = all(_fits_uint8(img[i:i + chunk_rows]) for i in range(0, len(img), chunk_rows))
    if not fits and image_storage == "uint8":
        raise ValueError("image_storage='uint8': some value is not float32(k) / 255 for a byte k")
    return "uint8" if fits else "float32"


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _device_ids(ids, n: int, device: torch.device) -> torch.Tensor:
    """``ids`` as a flat int32 device tensor.  Host ids (list, numpy, CPU tensor) outside ``[0, n)`` raise IndexError; a
    device tensor is passed through (the kernel clamps it)."""
    if isinstance(ids, torch.Tensor) and ids.is_cuda:
        if ids.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise TypeError(f"ids must be an integer tensor, got {ids.dtype}")
        return ids.to(device=device, dtype=torch.int32).reshape(-1).contiguous()        # the kernel clamps these
    h = np.asarray(ids.numpy() if isinstance(ids, torch.Tensor) else ids)
    if h.size and not np.issubdtype(h.dtype, np.integer):
        raise TypeError(f"ids must be integers, got {h.dtype}")
    h = h.reshape(-1).astype(np.int64)
    if h.size and (h.min() < 0 or h.max() >= n):
        raise IndexError(f"id {int(h[(h < 0) | (h >= n)][0])} outside [0, {n})")
    return torch.from_numpy(h.astype(np.int32)).to(device)


class FrameStore:
    """The image half of ``DeviceDataset``: ``img`` (T,96,96,3) with values ``pixel / 255.0`` (or uint8 pixels) kept in HBM,
    as uint8 where that is exact (``choose_image_storage``), uploaded ``_CHUNK_ROWS`` frames at a time.  ``frames(row_ids)``
    is ONE ``spdm_dataset_gather`` launch with one-row windows and no low-dimensional store."""

    def __init__(self, img, device: int = 0, image_storage: str = "auto"):
        img = np.asarray(img)
        if img.ndim != 4 or img.shape[1:] != FRAME_SHAPE or len(img) < 1:
            raise ValueError(f"expected img (T,96,96,3) with T >= 1, got {img.shape}")
        T = len(img)
        self.image_storage = choose_image_storage(img, image_storage)
        self.device = torch.device("cuda", device)
        self._T = T
        u8 = self.image_storage == "uint8"
        self._img = torch.empty((T,) + FRAME_SHAPE, dtype=torch.uint8 if u8 else torch.float32, device=self.device)
        for i in range(0, T, _CHUNK_ROWS):                                             # piecewise: the host never holds a second copy
            piece = img[i:i + _CHUNK_ROWS]
            if u8 and piece.dtype != np.uint8:
                piece = np.rint(piece * 255).astype(np.uint8)
            self._img[i:i + len(piece)] = torch.from_numpy(np.ascontiguousarray(piece, dtype=np.uint8 if u8 else np.float32)).to(self.device)
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)

    def __len__(self) -> int:
        return self._T

    def frames(self, row_ids) -> torch.Tensor:
        """``(n, 3, 96, 96)`` float32 frames of arbitrary store rows -- what ``autoencoder.training_step`` takes, enqueued on
        torch's current stream.  Host ids outside ``[0, len(self))`` raise IndexError; a device tensor is passed through and
        clamped by the kernel (``last_bad()``)."""
        ids = _device_ids(row_ids, self._T, self.device)
        if ids.numel() < 1:
            raise ValueError("an empty batch")
        out = torch.empty((ids.numel(), 3, 96, 96), dtype=torch.float32, device=self.device)
        a = _lib.SpdmDatasetGatherArgs(T=self._T, n_windows=self._T, B=ids.numel(), seq_len=1, step_size=1, n_frames=1,
                                       img_dtype=0 if self.image_storage == "uint8" else 1, reserved=0, d_img=self._img.data_ptr(),
                                       d_window_id=ids.data_ptr(), d_image_out=out.data_ptr(), d_bad=self._bad.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().spdm_dataset_gather(self.device.index, ctypes.byref(a), stream), "spdm_dataset_gather")
        return out

    def last_bad(self) -> int:
        """How many ids of the LAST ``frames`` call the kernel had to clamp into range.  Synchronises."""
        return int(self._bad.item())


def frames_to_u8(frames: torch.Tensor, out: Optional[torch.Tensor] = None, *, cols: int = 1, tile_offset: int = 0,
                 n_tiles: Optional[int] = None) -> torch.Tensor:
    """ONE ``spdm_frames_to_bytes`` launch on torch's current stream: the n planar fp32 ``frames`` (n,3,96,96)
    become the uint8 tiles ``tile_offset .. tile_offset + n - 1`` of the contact sheet ``out``, a contiguous uint8 device
    tensor ``(ceil(n_tiles / cols) * 96, cols * 96, 3)`` with ``cols`` tiles per row (made here, zero-filled, when None;
    ``n_tiles`` then defaults to ``tile_offset + n``).  The byte is ``clamp(rint(x * 255), 0, 255)`` in fp32, 0 for NaN; other
    tiles are not touched.  With ``cols=1`` the sheet viewed ``(n_tiles,96,96,3)`` is the image store's layout."""
    if frames.dim() != 4 or tuple(frames.shape[1:]) != (3, 96, 96) or not frames.is_cuda or frames.dtype != torch.float32 \
            or not frames.is_contiguous():
        raise ValueError(f"frames must be a contiguous (n,3,96,96) fp32 device tensor, got {tuple(frames.shape)} {frames.dtype}")
    n, cols, tile_offset = frames.shape[0], int(cols), int(tile_offset)
    if cols < 1:
        raise ValueError(f"cols = {cols} must be >= 1")
    if out is None:
        n_tiles = tile_offset + n if n_tiles is None else int(n_tiles)
        out = torch.zeros((-(-max(n_tiles, 1) // cols) * 96, cols * 96, 3), dtype=torch.uint8, device=frames.device)
    else:
        if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.dim() != 3 \
                or out.shape[1:] != (cols * 96, 3) or out.shape[0] % 96:
            raise ValueError(f"out must be a contiguous uint8 device tensor (rows * 96, cols * 96, 3), got {tuple(out.shape)}")
        held = out.shape[0] // 96 * cols
        n_tiles = held if n_tiles is None else int(n_tiles)
        if n_tiles > held:
            raise ValueError(f"n_tiles = {n_tiles}, out holds {held} tiles")
    a = _lib.SpdmFramesToBytesArgs(n=n, cols=cols, tile_offset=tile_offset, n_tiles=n_tiles, d_frames=frames.data_ptr(),
                                d_out=out.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(frames.device).cuda_stream)
    _lib.check(_lib.load().spdm_frames_to_bytes(frames.device.index, ctypes.byref(a), stream), "spdm_frames_to_bytes")
    return out


class DeviceDataset:
    """``CarRacingDataset`` (``stats=None``: the statistics are computed) or ``CarRacingDatasetForInference`` (``stats``
    given and used as they are) with every array on the device.

    ``position`` (T,2), ``velocity`` (T,2), ``action`` (T,3), ``img`` (T,96,96,3) with values ``pixel / 255.0`` (or uint8
    pixels), ``episode_ends``: the zarr groups' contents as numpy arrays.  Velocity and action are normalised here, once, by
    the reference's formula in the arrays' own precision and uploaded as float32; position is uploaded raw as float64 and
    normalised per window by the kernel.  ``image_storage``: see ``choose_image_storage``."""

    def __init__(self, position, velocity, action, img, episode_ends, pred_horizon: int, obs_horizon: int, step_size: int = 1,
                 stats: Optional[dict] = None, device: int = 0, image_storage: str = "auto"):
        position, velocity, action = np.asarray(position), np.asarray(velocity), np.asarray(action)
        img = np.asarray(img)
        T = len(position)
        if position.shape != (T, 2) or velocity.shape != (T, 2) or action.shape != (T, 3) or img.shape != (T,) + FRAME_SHAPE:
            raise ValueError(f"expected position (T,2), velocity (T,2), action (T,3), img (T,96,96,3); got {position.shape}, "
                             f"{velocity.shape}, {action.shape}, {img.shape}")
        self.obs_horizon, self.pred_horizon, self.step_size = int(obs_horizon), int(pred_horizon), int(step_size)
        self.sequence_len = self.obs_horizon + self.pred_horizon
        self.indices = create_sample_indices_sparse(episode_ends, self.sequence_len, self.step_size)
        if len(self.indices) == 0:
            raise ValueError("no episode holds a window of sequence_length * step_size rows")
        self.stats = stats if stats else compute_stats(position, velocity, action, self.indices, self.step_size)
        self._store = FrameStore(img, device, image_storage)                           # the image half: storage choice, upload
        self.image_storage, self.device, self._img, self._bad = self._store.image_storage, self._store.device, self._store._img, self._store._bad
        self._T = T
        self._pos_min, self._pos_max = float(self.stats["position"]["min"]), float(self.stats["position"]["max"])
        dev = self.device
        self._position = torch.from_numpy(np.ascontiguousarray(position, dtype=np.float64)).to(dev)
        self._velocity = torch.from_numpy(np.ascontiguousarray(normalize_data(velocity, self.stats["velocity"]), dtype=np.float32)).to(dev)
        self._action = torch.from_numpy(np.ascontiguousarray(normalize_data(action, self.stats["action"]), dtype=np.float32)).to(dev)
        self._h_start = np.ascontiguousarray(self.indices[:, 0], dtype=np.int32)      # the library checks this copy on the host
        self._d_start = torch.from_numpy(self._h_start).to(dev)

    def __len__(self) -> int:
        return len(self.indices)

    # ---- the one launch -------------------------------------------------------------------------------------------------------
    def _gather(self, ids: torch.Tensor, *, seq: int, step: int, n_frames: int, low: bool, translation: bool):
        B = ids.numel()
        if B < 1:
            raise ValueError("an empty batch")
        dev = self.device
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        out = {}
        if n_frames:
            out["image"] = f32(B, n_frames, 3, 96, 96)
        if low:
            out["position"], out["velocity"], out["action"] = f32(B, seq, 2), f32(B, seq, 2), f32(B, seq, 3)
        if translation:
            out["translation"] = torch.empty((B, 2), dtype=torch.float64, device=dev)
            out["start"] = torch.empty(B, dtype=torch.int32, device=dev)
        a = _lib.SpdmDatasetGatherArgs(
            T=self._T, n_windows=len(self.indices), B=B, seq_len=seq, step_size=step, n_frames=n_frames,
            img_dtype=0 if self.image_storage == "uint8" else 1, reserved=0,
            d_img=_ptr(self._img), d_position=_ptr(self._position), d_velocity=_ptr(self._velocity), d_action=_ptr(self._action),
            d_window_start=_ptr(self._d_start), h_window_start=self._h_start.ctypes.data,
            d_window_id=_ptr(ids), pos_min=self._pos_min, pos_max=self._pos_max,
            d_image_out=_ptr(out.get("image")), d_position_out=_ptr(out.get("position")), d_velocity_out=_ptr(out.get("velocity")),
            d_action_out=_ptr(out.get("action")), d_translation_out=_ptr(out.get("translation")), d_start_out=_ptr(out.get("start")),
            d_bad=_ptr(self._bad))
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().spdm_dataset_gather(dev.index, ctypes.byref(a), stream), "spdm_dataset_gather")
        return out

    def batch(self, window_ids, frames: Optional[str] = "obs", with_translation: bool = False) -> dict:
        """``{'image', 'position', 'velocity', 'action'}`` for the windows ``window_ids``: float32 device tensors
        ``(B, n_frames, 3, 96, 96)`` and ``(B, seq, 2 | 2 | 3)``, enqueued on torch's current stream.  ``frames``: ``'obs'``
        emits the first ``obs_horizon`` frames of each window (all that the model reads), ``'all'`` every frame as the
        reference does, ``None`` no ``'image'`` at all.  ``with_translation=True`` adds the inference flavour's
        ``'translation'`` (B,2) float64, ``'start'`` and ``'end'`` (B) int32.  Host ids (list, numpy, CPU tensor) outside
        ``[0, len(self))`` raise IndexError; a device tensor is passed through and clamped by the kernel (``last_bad()``)."""
        if frames not in ("obs", "all", None):
            raise ValueError(f"frames must be 'obs', 'all' or None, got {frames!r}")
        n_frames = {"obs": self.obs_horizon, "all": self.sequence_len, None: 0}[frames]
        out = self._gather(_device_ids(window_ids, len(self), self.device), seq=self.sequence_len, step=self.step_size,
                           n_frames=n_frames, low=True, translation=with_translation)
        if with_translation:
            out["end"] = out["start"] + self.sequence_len * self.step_size
        return out

    def frames(self, row_ids) -> torch.Tensor:
        """``(n, 3, 96, 96)`` float32 frames of arbitrary store rows -- what ``autoencoder.training_step`` takes.  The same
        kernel with one-row windows, window i starting at row i (``FrameStore.frames``)."""
        return self._store.frames(row_ids)

    def last_bad(self) -> int:
        """How many ids of the LAST ``batch`` / ``frames`` call the kernel had to clamp into range.  Synchronises."""
        return int(self._bad.item())


class _Batches:
    """A re-iterable over the batches of one id order; each batch dict also carries its ``'window_id'`` (device int32)."""

    def __init__(self, dataset: DeviceDataset, ids: np.ndarray, batch_size: int):
        self.dataset, self.window_ids, self.batch_size = dataset, np.asarray(ids, dtype=np.int64), int(batch_size)
        self._d_ids = torch.from_numpy(self.window_ids.astype(np.int32)).to(dataset.device)      # one upload per epoch order

    def __len__(self) -> int:
        return -(-len(self.window_ids) // self.batch_size)           # the last short batch is kept

    def __iter__(self):
        for i in range(0, len(self.window_ids), self.batch_size):
            ids = self._d_ids[i:i + self.batch_size]
            batch = self.dataset.batch(ids, frames="obs")
            batch["window_id"] = ids
            yield batch


class CarRacingDataModule:
    """The reference's data module (utils/load_data.py:146-182) over a ``DeviceDataset``: an 80 / 20 ``random_split`` and
    loaders that yield device batch dicts.  ``stats`` given selects the inference flavour, as there."""

    def __init__(self, batch_size: int, data_dir: Optional[str] = None, T_obs: int = 4, T_pred: int = 8, seed=None, stats=None,
                 step_size: int = 5, device: int = 0):
        self.batch_size, self.data_dir, self.T_obs, self.T_pred = int(batch_size), data_dir, T_obs, T_pred
        self.seed, self.stats, self.step_size, self.device = seed, stats, step_size, device
        self.data_full: Optional[DeviceDataset] = None

    def setup(self, name: Optional[str] = None, arrays: Optional[dict] = None) -> None:
        """``arrays``: ``{'position', 'velocity', 'action', 'img', 'episode_ends'}`` as numpy arrays.  ``name`` instead opens
        ``data_dir/name`` with zarr, as the reference does; zarr is imported only then, and that branch is NOT covered by the
        tests (zarr is not among the project's test dependencies)."""
        if (name is None) == (arrays is None):
            raise ValueError("pass either name (a zarr store under data_dir) or arrays")
        if arrays is None:
            try:
                import zarr
            except ImportError as e:
                raise ImportError("CarRacingDataModule.setup(name=...) reads a zarr store and needs the zarr package; "
                                  "pass arrays=... to use numpy arrays") from e
            root = zarr.open(os.path.join(self.data_dir or "", name), "r")
            arrays = {k: root["data"][k][:] for k in ("position", "velocity", "action", "img")}
            arrays["episode_ends"] = root["meta"]["episode_ends"][:]
        self.data_full = DeviceDataset(arrays["position"], arrays["velocity"], arrays["action"], arrays["img"],
                                       arrays["episode_ends"], self.T_pred, self.T_obs, step_size=self.step_size,
                                       stats=self.stats, device=self.device)
        self.stats = self.data_full.stats
        self.train_ids, self.val_ids = split_indices(len(self.data_full), self.seed)

    def train_dataloader(self, epoch: int = 0) -> _Batches:
        """The train split in a fresh random order per epoch: a ``torch.randperm`` from a generator seeded by
        ``(seed, epoch)``.  This order is this project's own: the reference's comes from the global RNG of its DataLoader
        and is not reproducible from ``seed`` either."""
        order = _epoch_order(len(self.train_ids), self.seed, epoch)
        return _Batches(self.data_full, self.train_ids[order], self.batch_size)

    def val_dataloader(self) -> _Batches:
        return _Batches(self.data_full, self.val_ids, self.batch_size)      # shuffle=False: the split's order

    def save_stats(self, path: str) -> None:
        with open(path, "wb") as f:
            pickle.dump([self.stats], f)


def _epoch_order(n: int, seed, epoch: int) -> np.ndarray:
    """A fresh order of ``n`` items for ``(seed, epoch)``: the loaders' one generator recipe."""
    g = torch.Generator().manual_seed((int(seed or 0) * 0x9E3779B1 + int(epoch)) & (2 ** 63 - 1))
    return torch.randperm(n, generator=g).numpy()


class _FrameBatches:
    """A sized re-iterable over the ``(B,3,96,96)`` float32 device batches of one row order of a frame store."""

    def __init__(self, store, ids: np.ndarray, batch_size: int):
        self.store, self.row_ids, self.batch_size = store, np.asarray(ids, dtype=np.int64), int(batch_size)
        self._d_ids = None

    def __len__(self) -> int:
        return -(-len(self.row_ids) // self.batch_size)              # the last short batch is kept

    def __iter__(self):
        if self._d_ids is None:                                      # one upload per order
            self._d_ids = torch.from_numpy(self.row_ids.astype(np.int32)).to(self.store.device)
        for i in range(0, len(self.row_ids), self.batch_size):
            yield self.store.frames(self._d_ids[i:i + self.batch_size])


class FramesDataModule:
    """The reference's ``ImagesDataset`` + ``DataModule`` of models/encoder/train_autoencoder.py:24-61 over a ``FrameStore``:
    every frame of the store is a sample, an 80 / 20 ``random_split``, loaders that yield ``(B,3,96,96)`` float32 device
    batches.  There are no statistics: the autoencoder's run writes no STATS.pkl, as in the reference."""

    def __init__(self, batch_size: int, data_dir: Optional[str] = None, seed=None, device: int = 0, image_storage: str = "auto"):
        self.batch_size, self.data_dir, self.seed, self.device, self.image_storage = int(batch_size), data_dir, seed, device, image_storage
        self.data_full = None

    def setup(self, name: Optional[str] = None, arrays: Optional[dict] = None, store=None) -> None:
        """``arrays``: ``{'img': (T,96,96,3)}`` (other keys are ignored, so the arrays of ``CarRacingDataModule`` serve).
        ``name`` instead opens ``data_dir/name`` with zarr, imported only then and NOT covered by the tests.  ``store``: a
        ready ``FrameStore`` (or anything with ``frames(ids)``, ``device`` and ``__len__``)."""
        if (name is None) + (arrays is None) + (store is None) != 2:
            raise ValueError("pass exactly one of name (a zarr store under data_dir), arrays and store")
        if name is not None:
            try:
                import zarr
            except ImportError as e:
                raise ImportError("FramesDataModule.setup(name=...) reads a zarr store and needs the zarr package; "
                                  "pass arrays=... to use numpy arrays") from e
            arrays = {"img": zarr.open(os.path.join(self.data_dir or "", name), "r")["data"]["img"][:]}
        self.data_full = store if store is not None else FrameStore(arrays["img"], self.device, self.image_storage)
        self.train_ids, self.val_ids = split_indices(len(self.data_full), self.seed)

    def train_dataloader(self, epoch: int = 0) -> _FrameBatches:
        """The train split in a fresh ``(seed, epoch)`` order, ``CarRacingDataModule.train_dataloader``'s recipe."""
        return _FrameBatches(self.data_full, self.train_ids[_epoch_order(len(self.train_ids), self.seed, epoch)], self.batch_size)

    def val_dataloader(self) -> _FrameBatches:
        return _FrameBatches(self.data_full, self.val_ids, self.batch_size)      # shuffle=False: the split's order


__all__ = ["FrameStore", "FramesDataModule", "frames_to_u8", "create_sample_indices_sparse", "compute_stats", "normalize_data", "unnormalize_data", "unnormalize_position", "split_indices",
           "choose_image_storage", "DeviceDataset", "CarRacingDataModule"]
