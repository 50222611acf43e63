"""The host side of the autoencoder's run without a GPU: FramesDataModule's split and epoch orders over a
stub store, both command lines' defaults against the reference's settings, the PPM writer, and train.fit with and without a
data module's ``save_stats``."""
import os

import numpy as np
import torch

from state_policy_diffusionmodel_amd import eval_autoencoder, train_autoencoder
from state_policy_diffusionmodel_amd.dataset import FramesDataModule, split_indices
from state_policy_diffusionmodel_amd.train import fit

from test_fit_loop import StubData, StubModel


class StubStore:
    """``FrameStore``'s surface on the host: frame i is filled with the value i."""
    device = "cpu"

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def frames(self, ids):
        return ids.to(torch.float32).view(-1, 1, 1, 1).expand(-1, 3, 96, 96)


def _dm(seed=7, batch=8, n=40):
    dm = FramesDataModule(batch, seed=seed)
    dm.setup(store=StubStore(n))
    return dm


def _rows(loader):
    return [b[:, 0, 0, 0].to(torch.int64).tolist() for b in loader]


def test_split_and_orders_are_reproducible_from_seed_and_epoch():
    dm, again = _dm(), _dm()
    train, val = split_indices(40, 7)
    assert np.array_equal(dm.train_ids, train) and np.array_equal(dm.val_ids, val)
    assert len(dm.train_ids) == 32 and len(dm.val_ids) == 8 and sorted(list(train) + list(val)) == list(range(40))
    e0, e1 = dm.train_dataloader(0), dm.train_dataloader(1)
    assert len(e0) == 4 and len(dm.val_dataloader()) == 1
    assert _rows(e0) == _rows(e0) == _rows(again.train_dataloader(0))         # re-iterable, and a function of (seed, epoch)
    assert _rows(e1) == _rows(again.train_dataloader(1)) and _rows(e1) != _rows(e0)
    assert sorted(sum(_rows(e0), [])) == sorted(train.tolist()) == sorted(sum(_rows(e1), []))
    assert sum(_rows(dm.val_dataloader()), []) == val.tolist()                # shuffle=False: the split's order
    assert np.array_equal(dm.val_dataloader().row_ids, val)
    assert _rows(_dm(seed=8).train_dataloader(0)) != _rows(e0)
    batch = next(iter(e0))
    assert batch.shape == (8, 3, 96, 96) and batch.dtype == torch.float32


def test_the_last_short_batch_is_kept():
    dm = _dm(batch=5, n=41)                                                   # 32 train rows: 6 batches of 5 and one of 2
    sizes = [b.shape[0] for b in dm.train_dataloader(3)]
    assert sizes == [5] * 6 + [2] and len(dm.train_dataloader(3)) == 7
    assert [b.shape[0] for b in dm.val_dataloader()] == [5, 4]


def test_setup_takes_exactly_one_source():
    dm = FramesDataModule(8)
    for kw in ({}, {"name": "x", "store": StubStore(4)}):
        try:
            dm.setup(**kw)
        except ValueError as e:
            assert "exactly one" in str(e)
        else:
            raise AssertionError(kw)


def test_parser_defaults_are_the_references_settings():
    """models/encoder/train_autoencoder.py:64-89: batch_size=128, n_epochs = 50, autoencoder()'s learning_rate 1e-3,
    val_check_interval=0.5, gradient_clip_val=0.5, EarlyStopping(monitor='lr', stopping_threshold=2e-6, patience=n_epochs)."""
    a = train_autoencoder.build_parser().parse_args(["--arrays", "x.npz"])
    assert (a.batch_size, a.n_epochs, a.lr, a.out_dir, a.seed) == (128, 50, 1e-3, "runs/autoencoder", 0)
    assert a.ckpt_path is None and a.dataset is None and not a.no_early_stop and a.image_storage == "auto"
    assert (train_autoencoder.VAL_CHECK_INTERVAL, train_autoencoder.GRADIENT_CLIP_VAL, train_autoencoder.LR_STOPPING_THRESHOLD) == (0.5, 0.5, 2e-6)
    assert not hasattr(a, "ema")
    e = eval_autoencoder.build_parser().parse_args(["--checkpoint", "c.ckpt", "--arrays", "x.npz"])
    assert (e.split, e.columns, e.sheet_frames, e.out, e.sheet, e.terms, e.seed) == ("val", 8, 8, None, None, False, 0)


def test_main_hands_fit_the_references_trainer_settings(monkeypatch, tmp_path):
    import state_policy_diffusionmodel_amd.autoencoder as ae
    import state_policy_diffusionmodel_amd.dataset as ds
    seen = {}
    monkeypatch.setattr(ae, "autoencoder", lambda **kw: seen.setdefault("model", kw) and "MODEL")
    monkeypatch.setattr(ds, "FrameStore", lambda img, device, storage: StubStore(len(img)))
    monkeypatch.setattr(train_autoencoder, "fit", lambda model, dm, **kw: seen.update(fit=kw, dm=dm) or {"ok": True})
    npz = str(tmp_path / "frames.npz")
    np.savez(npz, img=np.zeros((10, 96, 96, 3), np.uint8), position=np.zeros((10, 2)))      # other keys are ignored
    assert train_autoencoder.main(["--arrays", npz, "--n_epochs", "30", "--out_dir", str(tmp_path), "--seed", "4"]) == {"ok": True}
    kw = seen["fit"]
    assert seen["model"] == {"learning_rate": 1e-3, "weight_seed": 4}
    assert (kw["max_epochs"], kw["val_check_interval"], kw["gradient_clip_val"], kw["validate_first"], kw["device_optimizer"]) == (30, 0.5, 0.5, True, True)
    assert (kw["early_stop"].threshold, kw["early_stop"].patience, kw["seed"], kw["ckpt_path"]) == (2e-6, 30, 4, None)
    assert "ema" not in kw and len(seen["dm"].train_ids) == 8 and seen["dm"].batch_size == 128


def test_ppm_header_and_byte_order(tmp_path):
    pix = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)               # H = 2, W = 3
    path = str(tmp_path / "s.ppm")
    eval_autoencoder.write_ppm(path, pix)
    raw = open(path, "rb").read()
    assert raw == b"P6\n3 2\n255\n" + bytes(range(18))                        # width first; rows top to bottom, R G B per pixel
    try:
        eval_autoencoder.write_ppm(path, pix.astype(np.float32))
    except ValueError:
        pass
    else:
        raise AssertionError("float pixels were accepted")


class NoStatsData:
    """A data module without ``save_stats``, as FramesDataModule"""
    batch_size = 8

    def train_dataloader(self, epoch):
        return [(epoch, i) for i in range(2)]

    def val_dataloader(self):
        return "VAL"


def test_fit_runs_against_a_data_module_without_save_stats(tmp_path):
    assert not hasattr(FramesDataModule, "save_stats")
    model = StubModel("autoencoder")
    res = fit(model, NoStatsData(), max_epochs=1, out_dir=tmp_path, val_check_interval=0.5, validate_first=True)
    assert sorted(os.listdir(tmp_path)) == ["checkpoints", "hparams.yaml", "metrics.jsonl"]
    assert [(x["kind"], x["epoch"], x["global_step"]) for x in res["metrics"]] == [("val", -1, 0), ("val", 0, 1), ("val", 0, 2), ("epoch", 0, 2)]
    steps = [e[2] for e in model.events if e[0] == "train"]               # what the loop passes a model named 'autoencoder'
    assert [sorted(kw) for kw in steps] == [["backward", "device_noise", "noise_step", "seed", "time_dropout"]] * 2


def test_fit_still_writes_the_stats_of_a_data_module_that_has_them(tmp_path):
    fit(StubModel(), StubData(2), max_epochs=1, out_dir=tmp_path)
    assert open(os.path.join(str(tmp_path), "STATS.pkl"), "rb").read() == b"stats"
