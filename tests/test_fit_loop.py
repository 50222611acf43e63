"""train.fit on the CPU with stub model and data objects that record what the loop asks of them, against hand-worked
expectations: where validation runs, what the scheduler and the early stop see, which files appear, what the log says, and
that a resumed run continues as the uninterrupted one would."""
import json
import os

import pytest
import torch

from state_policy_diffusionmodel_amd.train import LrEarlyStop, fit, main, validation_points


class StubOptimizer:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]

    def state_dict(self):
        return {"lr": self.param_groups[0]["lr"]}

    def load_state_dict(self, sd):
        self.param_groups[0]["lr"] = sd["lr"]


class StubScheduler:
    """Divides the lr by ``factor`` at the step calls whose 0-based number is in ``reduce_at``."""

    def __init__(self, optimizer, reduce_at=(), factor=10.0):
        self.optimizer, self.reduce_at, self.factor = optimizer, set(reduce_at), factor
        self.calls = []

    def step(self, metric):
        if len(self.calls) in self.reduce_at:
            self.optimizer.param_groups[0]["lr"] /= self.factor
        self.calls.append(metric)

    def state_dict(self):
        return {"calls": list(self.calls)}

    def load_state_dict(self, sd):
        self.calls = list(sd["calls"])


class StubModel:
    """Loss of training step g is 1 + g; val_loss after s optimiser steps is 8 - s / 8 (both exact in fp32 / fp64)."""
    device = "cpu"

    def __init__(self, model_name="UNet_FilmnoAttention", lr=0.5, reduce_at=(), factor=10.0):
        self.model_name, self.lr, self.reduce_at, self.factor = model_name, lr, reduce_at, factor
        self.steps = 0
        self.events = []
        self.restored = None

    def configure_optimizers(self, device_optimizer=False):
        self.device_optimizer = device_optimizer
        self.optimizer = StubOptimizer(self.lr)
        self.scheduler = StubScheduler(self.optimizer, self.reduce_at, self.factor)
        return {"optimizer": self.optimizer, "lr_scheduler": {"scheduler": self.scheduler, "monitor": "val_loss", "frequency": 1}}

    def training_step(self, batch, **kw):
        self.events.append(("train", batch, kw))
        return torch.tensor(1.0 + kw["noise_step"])

    def optimizer_step(self, optimizer, gradient_clip_val):
        assert optimizer is self.optimizer
        self.events.append(("opt", gradient_clip_val))
        self.steps += 1

    def validation_loss(self, batches, *, seed):
        self.events.append(("val", batches, seed))
        return 8.0 - self.steps / 8.0

    def save_checkpoint(self, path, *, optimizer, scheduler, trainer_state):
        self.events.append(("ckpt", os.path.basename(path)))
        torch.save({"state_dict": {"steps": self.steps}, "optimizer_states": [optimizer.state_dict()],
                    "lr_schedulers": [scheduler.state_dict()], "spdm_trainer": dict(trainer_state)}, path)

    def save_hparams(self, path):
        open(path, "w").write("model: stub\n")

    def restore_checkpoint(self, ckpt):
        self.restored = ckpt
        self.steps = ckpt["state_dict"]["steps"]


class StubData:
    batch_size = 8

    def __init__(self, n_train_batches):
        self.n = n_train_batches
        self.epochs = []

    def train_dataloader(self, epoch):
        self.epochs.append(epoch)
        return [(epoch, i) for i in range(self.n)]

    def val_dataloader(self):
        return "VAL"

    def save_stats(self, path):
        open(path, "wb").write(b"stats")


def _lines(out_dir):
    return [json.loads(line) for line in open(os.path.join(str(out_dir), "metrics.jsonl"))]


# hand-worked: every = max(1, int(n * 0.25)) is 1 for n = 1, 3, 4, 6 (int(0.25), int(0.75), int(1.0), int(1.5)) and 2 for n = 10
POINTS = {1: [0], 3: [0, 1, 2], 4: [0, 1, 2, 3], 6: [0, 1, 2, 3, 4, 5], 10: [1, 3, 5, 7, 9]}


@pytest.mark.parametrize("n", sorted(POINTS))
def test_validation_points_at_a_quarter(n, tmp_path):
    assert validation_points(n, 0.25) == POINTS[n]
    m, d = StubModel(), StubData(n)
    fit(m, d, max_epochs=1, out_dir=tmp_path, validate_first=False, seed=3)
    seen, i = [], -1
    for ev in m.events:
        if ev[0] == "train":
            i += 1
            assert ev[1] == (0, i)
        elif ev[0] == "val":
            assert ev[1:] == ("VAL", 3)
            seen.append(i)
    assert seen == POINTS[n] and i == n - 1


def test_validation_points_other_intervals():
    assert validation_points(5, 0.5) == [1, 3] and validation_points(5, 1.0) == [4] and validation_points(5, 7) == []
    assert validation_points(5, 2) == [1, 3]
    with pytest.raises(ValueError):
        validation_points(5, 0.0)
    with pytest.raises(ValueError):
        validation_points(5, 1.5)


def test_steps_scheduler_checkpoints_and_log(tmp_path):
    """5 train batches, interval 0.5 (every 2), 2 epochs, lr 0.5 divided by 10 at the first scheduler step."""
    m, d = StubModel(reduce_at=(0,)), StubData(5)
    res = fit(m, d, max_epochs=2, out_dir=tmp_path, val_check_interval=0.5, gradient_clip_val=0.25, seed=9)
    assert m.device_optimizer is True and d.epochs == [0, 1]
    trains = [e for e in m.events if e[0] == "train"]
    assert [e[1] for e in trains] == [(0, i) for i in range(5)] + [(1, i) for i in range(5)]
    for g, e in enumerate(trains):           # one noise key per step over the whole run; no dropout keyword for a FiLM model
        assert e[2] == dict(backward=True, device_noise=True, seed=9, noise_step=g)
    assert [e for e in m.events if e[0] == "opt"] == [("opt", 0.25)] * 10
    kinds = [e[0] for e in m.events]
    assert kinds[0] == "val"                                                  # validate_first
    assert all(kinds[i + 1] == "opt" for i, k in enumerate(kinds) if k == "train")
    assert m.scheduler.calls == [7.5, 6.875]                                  # once per epoch, the epoch's latest val_loss
    assert [e[1] for e in m.events if e[0] == "ckpt"] == ["epoch=0.ckpt", "epoch=1.ckpt"]
    assert sorted(os.listdir(tmp_path / "checkpoints")) == ["epoch=0.ckpt", "epoch=1.ckpt"]
    assert open(tmp_path / "STATS.pkl", "rb").read() == b"stats" and open(tmp_path / "hparams.yaml").read() == "model: stub\n"
    L = lambda kind, epoch, gs, val, lr, tl: dict(kind=kind, epoch=epoch, global_step=gs, val_loss=val, lr=lr, train_loss=tl)  # noqa: E731
    want = [L("val", -1, 0, 8.0, 0.5, None),
            L("val", 0, 2, 7.75, 0.5, 1.5), L("val", 0, 4, 7.5, 0.5, 3.5), L("epoch", 0, 5, 7.5, 0.05, 5.0),
            L("val", 1, 7, 7.125, 0.05, 6.5), L("val", 1, 9, 6.875, 0.05, 8.5), L("epoch", 1, 10, 6.875, 0.05, 10.0)]
    assert _lines(tmp_path) == want and res["metrics"] == want
    assert res["epoch"] == 1 and res["global_step"] == 10 and res["val_loss"] == 6.875 and res["lr"] == 0.05 and not res["stopped_early"]
    st = torch.load(tmp_path / "checkpoints" / "epoch=1.ckpt", weights_only=True)["spdm_trainer"]
    assert st == dict(epoch=1, global_step=10, val_loss=6.875, seed=9, early_stop=None, stopped_early=False)


def test_simple_unet_trains_with_time_dropout(tmp_path):
    m = StubModel(model_name="UNet")
    fit(m, StubData(2), max_epochs=1, out_dir=tmp_path, validate_first=False)
    assert [e[2]["time_dropout"] for e in m.events if e[0] == "train"] == [0.1, 0.1]
    assert not os.path.exists(tmp_path / "checkpoints" / "epoch=1.ckpt")
    assert _lines(tmp_path)[0]["epoch"] == 0                                  # no validation before training


def test_early_stop_rule():
    s = LrEarlyStop(0.5, 100)
    assert not s.check(0.5)                                                   # strictly below only
    assert s.check(0.4999) and "stopping_threshold" in s.reason
    s = LrEarlyStop(1e-4, 3)
    assert [s.check(0.5), s.check(0.5), s.check(0.5)] == [False, False, False] and s.wait == 2
    assert not s.check(0.25) and s.wait == 0 and s.best == 0.25              # a decrease resets the count
    assert [s.check(0.25), s.check(0.25), s.check(0.25)] == [False, False, True] and "patience" in s.reason
    t = LrEarlyStop(1e-4, 3)
    t.load_state_dict(s.state_dict())
    assert (t.best, t.wait) == (0.25, 3)


def test_early_stop_at_the_first_validation_below_the_threshold(tmp_path):
    """lr 0.5 -> 0.05 at the end of epoch 0; threshold 0.1: the first validation of epoch 1 (after its 2nd batch) stops the run."""
    m = StubModel(reduce_at=(0,))
    res = fit(m, StubData(5), max_epochs=4, out_dir=tmp_path, val_check_interval=0.5, early_stop=LrEarlyStop(0.1, 100))
    assert res["stopped_early"] and res["epoch"] == 1 and res["global_step"] == 7
    assert [(x["kind"], x["epoch"], x["global_step"]) for x in _lines(tmp_path)][-2:] == [("val", 1, 7), ("epoch", 1, 7)]
    assert len(m.scheduler.calls) == 2                                        # the stopped epoch still ends: scheduler, log, checkpoint
    assert sorted(os.listdir(tmp_path / "checkpoints")) == ["epoch=0.ckpt", "epoch=1.ckpt"]
    assert torch.load(tmp_path / "checkpoints" / "epoch=1.ckpt", weights_only=True)["spdm_trainer"]["stopped_early"] is True


def test_early_stop_after_patience_validations_without_a_decrease(tmp_path):
    """2 batches, a validation after each; patience 3; lr halves at the end of epoch 0.  Counts: e0 0, 1 | e1 0 (decrease), 1 |
    e2 2, 3 -> stop at the 2nd validation of epoch 2.  Without the reset the run would have stopped in epoch 1."""
    m = StubModel(reduce_at=(0,), factor=2.0)
    es = LrEarlyStop(1e-4, 3)
    res = fit(m, StubData(2), max_epochs=9, out_dir=tmp_path, val_check_interval=0.5, early_stop=es)
    assert res["stopped_early"] and res["epoch"] == 2 and res["global_step"] == 6 and es.wait == 3 and es.best == 0.25
    m = StubModel()                                                           # lr constant: 0, 1, 2, 3 -> the 4th validation
    res = fit(m, StubData(2), max_epochs=9, out_dir=tmp_path / "b", val_check_interval=0.5, early_stop=LrEarlyStop(1e-4, 3))
    assert res["stopped_early"] and res["epoch"] == 1 and res["global_step"] == 4
    m = StubModel()                                                           # no early stop by default
    assert not fit(m, StubData(2), max_epochs=3, out_dir=tmp_path / "c")["stopped_early"]


def test_resume_restores_every_counter(tmp_path):
    kw = dict(val_check_interval=0.5, seed=4)
    one, d1 = StubModel(reduce_at=(1,), factor=2.0), StubData(5)
    es1 = LrEarlyStop(1e-4, 50)
    fit(one, d1, max_epochs=3, out_dir=tmp_path / "a", early_stop=es1, **kw)

    first = StubModel(reduce_at=(1,), factor=2.0)
    fit(first, StubData(5), max_epochs=2, out_dir=tmp_path / "b", early_stop=LrEarlyStop(1e-4, 50), **kw)
    second, d2, es2 = StubModel(reduce_at=(1,), factor=2.0), StubData(5), LrEarlyStop(1e-4, 50)
    res = fit(second, d2, max_epochs=3, out_dir=tmp_path / "b", early_stop=es2, ckpt_path=tmp_path / "b" / "checkpoints" / "epoch=1.ckpt", **kw)
    assert second.restored is not None and second.restored["spdm_trainer"]["epoch"] == 1
    assert d2.epochs == [2]                                                   # continues at the next epoch, no validation first
    assert second.events[0][0] == "train" and second.events[0][2]["noise_step"] == 10
    assert [e for e in second.events if e[0] == "train"] == [e for e in one.events if e[0] == "train"][10:]
    assert second.optimizer.param_groups[0]["lr"] == one.optimizer.param_groups[0]["lr"] == 0.25
    assert second.scheduler.calls == one.scheduler.calls and len(one.scheduler.calls) == 3
    assert (es2.best, es2.wait) == (es1.best, es1.wait)
    assert _lines(tmp_path / "b") == _lines(tmp_path / "a")                   # the resumed run appends to the log
    assert res["global_step"] == 15 and res["epoch"] == 2
    a = torch.load(tmp_path / "a" / "checkpoints" / "epoch=2.ckpt", weights_only=True)
    b = torch.load(tmp_path / "b" / "checkpoints" / "epoch=2.ckpt", weights_only=True)
    assert a == b


def test_resume_restores_the_latest_val_loss(tmp_path):
    """An interval longer than the epoch: only the validation before training runs, and every epoch's scheduler step -- the
    resumed one's too -- sees that value."""
    m = StubModel()
    fit(m, StubData(3), max_epochs=1, out_dir=tmp_path, val_check_interval=7)
    assert m.scheduler.calls == [8.0]
    r = StubModel()
    res = fit(r, StubData(3), max_epochs=2, out_dir=tmp_path, val_check_interval=7, ckpt_path=tmp_path / "checkpoints" / "epoch=0.ckpt")
    assert r.scheduler.calls == [8.0, 8.0] and res["val_loss"] == 8.0 and not [e for e in r.events if e[0] == "val"]
    with pytest.raises(ValueError, match="seed"):
        fit(StubModel(), StubData(3), max_epochs=2, out_dir=tmp_path, seed=1, ckpt_path=tmp_path / "checkpoints" / "epoch=0.ckpt")
    torch.save({"state_dict": {}}, tmp_path / "foreign.ckpt")
    with pytest.raises(ValueError, match="spdm_trainer"):
        fit(StubModel(), StubData(3), max_epochs=2, out_dir=tmp_path, ckpt_path=tmp_path / "foreign.ckpt")


def test_amp_is_refused_with_a_clear_message(capsys):
    with pytest.raises(SystemExit) as e:
        main(["--amp", "--arrays", "nowhere.npz"])
    assert e.value.code != 0
    assert "exact fp32" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main([])                                                              # neither --dataset nor --arrays
