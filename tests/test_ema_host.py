"""The host side of the EMA of the weights without a GPU: DeviceEMA's state dict, what train.fit asks of a
model when ``ema=`` is given -- and that it asks nothing new when it is not --, and the checkpoint's two new keys."""
import json
import os
import types

import numpy as np
import pytest
import torch

from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM, _index_of, load_model
from state_policy_diffusionmodel_amd.optim import EMA_SCHEDULE, DeviceEMA, ema_decay
from state_policy_diffusionmodel_amd.train import build_parser, fit
from state_policy_diffusionmodel_amd.weights import pack_state_dict
from test_fit_loop import StubData, StubModel


# ---- DeviceEMA's state ----------------------------------------------------------------------------------------------------------
def _host_ema(sizes=(5, 12), step=3, **schedule):
    """A DeviceEMA with host tensors in the places of its device ones (its constructor needs the GPU; its state does not)."""
    ema = object.__new__(DeviceEMA)
    g = torch.Generator().manual_seed(sum(sizes) + step)
    ema.params = [torch.randn(n, generator=g) for n in sizes]
    ema.shadow = [torch.randn(n, generator=g) for n in sizes]
    ema.schedule = dict(EMA_SCHEDULE, **schedule)
    ema.optimization_step = step
    return ema


def test_state_dict_round_trip():
    a, b = _host_ema(step=41, max_value=0.99), _host_ema(step=0, max_value=0.99)
    sd = a.state_dict()
    assert sorted(sd) == ["optimization_step", "schedule", "shadow"] and sd["optimization_step"] == 41
    assert sd["schedule"] == dict(EMA_SCHEDULE, max_value=0.99)
    assert not torch.equal(a.shadow[1], b.shadow[1])
    kept = [s.data_ptr() for s in b.shadow]
    b.load_state_dict(sd)
    assert b.optimization_step == 41 and all(torch.equal(x, y) for x, y in zip(a.shadow, b.shadow))
    assert [s.data_ptr() for s in b.shadow] == kept                           # copied in: the tensors a launch writes stay
    b.shadow[0].zero_()
    assert a.shadow[0].abs().sum() > 0                                        # ... and are not the source's


def test_load_refuses_another_schedule_or_shape():
    a = _host_ema()
    with pytest.raises(ValueError, match="schedule"):
        _host_ema(power=0.5).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="shadow"):
        _host_ema(sizes=(5, 13)).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="shadow"):
        _host_ema(sizes=(5,)).load_state_dict(a.state_dict())


def test_constructor_checks_its_arguments_as_device_adam_does():
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="on the GPU"):
        DeviceEMA([p])
    with pytest.raises(ValueError, match="1 to 4"):
        DeviceEMA([])
    with pytest.raises(ValueError, match="1 to 4"):
        DeviceEMA([p] * 5)
    with pytest.raises(TypeError, match="decay"):
        DeviceEMA([p], decay=0.9)


# ---- fit ------------------------------------------------------------------------------------------------------------------------
class EmaStubModel(StubModel):
    """StubModel with an EMA: val_loss_ema after s optimiser steps is 4 - s / 16."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ema_calls = []
        self.ema = None

    def configure_ema(self, **schedule):
        self.ema_calls.append(schedule)
        self.ema = types.SimpleNamespace(optimization_step=self.steps)
        return self.ema

    def optimizer_step(self, optimizer, gradient_clip_val):
        super().optimizer_step(optimizer, gradient_clip_val)
        if self.ema is not None:
            self.ema.optimization_step += 1

    def validation_loss(self, batches, *, seed, use_ema=False):
        if use_ema:
            self.events.append(("val_ema", batches, seed))
            return 4.0 - self.steps / 16.0
        return super().validation_loss(batches, seed=seed)

    def restore_checkpoint(self, ckpt):
        super().restore_checkpoint(ckpt)
        self.ema.optimization_step = self.steps


class NoEmaModel(StubModel):
    def __getattr__(self, name):
        if name == "configure_ema":
            raise AssertionError("fit() without ema= looked configure_ema up")
        raise AttributeError(name)


def _lines(out_dir):
    return [json.loads(line) for line in open(os.path.join(str(out_dir), "metrics.jsonl"))]


def test_fit_without_ema_never_touches_configure_ema(tmp_path):
    m = NoEmaModel()
    res = fit(m, StubData(4), max_epochs=1, out_dir=tmp_path, val_check_interval=0.5)
    assert all(sorted(x) == ["epoch", "global_step", "kind", "lr", "train_loss", "val_loss"] for x in _lines(tmp_path))
    assert "val_loss_ema" not in res
    st = torch.load(tmp_path / "checkpoints" / "epoch=0.ckpt", weights_only=True)["spdm_trainer"]
    assert sorted(st) == ["early_stop", "epoch", "global_step", "seed", "stopped_early", "val_loss"]
    with pytest.raises(ValueError, match="ema_monitor"):
        fit(StubModel(), StubData(4), max_epochs=1, out_dir=tmp_path, ema_monitor=True)


def test_fit_with_ema_configures_once_and_logs_both_losses(tmp_path):
    m = EmaStubModel()
    sched = {"max_value": 0.99, "power": 0.5}
    res = fit(m, StubData(4), max_epochs=2, out_dir=tmp_path, val_check_interval=0.5, seed=2, ema=sched)
    assert m.ema_calls == [sched]
    kinds = [e[0] for e in m.events if e[0] in ("val", "val_ema")]
    assert kinds == ["val", "val_ema"] * 5                                    # every validation: the live pass, then the averaged one
    assert all(e[1:] == ("VAL", 2) for e in m.events if e[0] == "val_ema")
    lines = _lines(tmp_path)
    assert lines == res["metrics"] and len(lines) == 7
    want = [(-1, 0), (0, 2), (0, 4), (0, 4), (1, 6), (1, 8), (1, 8)]
    for line, (epoch, steps) in zip(lines, want):
        assert (line["epoch"], line["global_step"]) == (epoch, steps)
        assert line["val_loss"] == 8.0 - steps / 8.0 and line["val_loss_ema"] == 4.0 - steps / 16.0
        assert line["ema_decay"] == ema_decay(steps, **sched)
    assert m.scheduler.calls == [7.5, 7.0]                                    # the scheduler follows val_loss ...
    assert res["val_loss_ema"] == 3.5
    st = torch.load(tmp_path / "checkpoints" / "epoch=1.ckpt", weights_only=True)["spdm_trainer"]
    assert st["val_loss_ema"] == 3.5 and st["val_loss"] == 7.0


def test_ema_monitor_makes_the_scheduler_follow_val_loss_ema(tmp_path):
    m = EmaStubModel()
    fit(m, StubData(4), max_epochs=2, out_dir=tmp_path, val_check_interval=0.5, ema={}, ema_monitor=True)
    assert m.ema_calls == [{}] and m.scheduler.calls == [3.75, 3.5]


def test_resumed_fit_restores_the_latest_val_loss_ema(tmp_path):
    """An interval longer than the epoch: the only validation is the one before training, and the resumed epoch's scheduler step
    sees its val_loss_ema from the checkpoint."""
    kw = dict(val_check_interval=7, ema={}, ema_monitor=True)
    fit(EmaStubModel(), StubData(3), max_epochs=1, out_dir=tmp_path, **kw)
    r = EmaStubModel()
    res = fit(r, StubData(3), max_epochs=2, out_dir=tmp_path, ckpt_path=tmp_path / "checkpoints" / "epoch=0.ckpt", **kw)
    assert r.ema_calls == [{}] and r.scheduler.calls == [4.0, 4.0] and res["val_loss_ema"] == 4.0
    assert [x["ema_decay"] for x in _lines(tmp_path)] == [0.0, ema_decay(3), ema_decay(6)]


def test_train_command_line_has_the_ema_flags():
    a = build_parser().parse_args(["--arrays", "x.npz"])
    assert (a.ema, a.ema_monitor, a.ema_max_decay, a.ema_power, a.ema_inv_gamma, a.ema_update_after_step) == (False, False, 0.9999, 0.75, 1.0, 0)
    a = build_parser().parse_args(["--arrays", "x.npz", "--ema", "--ema_max_decay", "0.999", "--ema_power", "0.6", "--ema_inv_gamma", "2",
                                   "--ema_update_after_step", "10", "--ema_monitor"])
    assert (a.ema, a.ema_monitor, a.ema_max_decay, a.ema_power, a.ema_inv_gamma, a.ema_update_after_step) == (True, True, 0.999, 0.6, 2.0, 10)


@pytest.mark.parametrize("module", ["generate", "evaluate", "run_predictions"])
def test_inference_command_lines_take_use_ema(module):
    import importlib
    mod = importlib.import_module("state_policy_diffusionmodel_amd." + module)
    base = [] if module == "generate" else ["--checkpoint", "c", "--hparams", "h", "--data", "d"] + (["--stats", "s"] if module == "run_predictions" else [])
    assert mod.parse_arguments(base).use_ema is False and mod.parse_arguments(base + ["--use_ema"]).use_ema is True


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------
HP = dict(noise_steps=50, obs_horizon=2, pred_horizon=6, observation_dim=10, prediction_dim=3, learning_rate=3e-4,
          noise_scheduler_type="linear", inpaint_horizon=2, step_size=5)


def _model_with_host_ema():
    """A model (no engine, no device) whose EMA is a stand-in with a host shadow: the live weights scaled by 1/2."""
    m = Diffusion_DDPM(model="UNet_FilmnoAttention", weight_seed=5, **HP)
    blob, idx = pack_state_dict(m.noise_estimator._host_sd)
    m.noise_estimator._flat_index = _index_of(idx)
    m._ema = types.SimpleNamespace(shadow=[torch.from_numpy(blob.copy()) * 0.5], optimization_step=17,
                                   schedule=dict(EMA_SCHEDULE, max_value=0.999))
    return m


def test_checkpoint_with_an_ema_carries_two_new_keys_and_loads_safely(tmp_path):
    m = _model_with_host_ema()
    with_ema, without = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    m.save_checkpoint(with_ema, trainer_state={"epoch": 0, "global_step": 17})
    plain = Diffusion_DDPM(model="UNet_FilmnoAttention", weight_seed=5, **HP)
    plain.save_checkpoint(without, trainer_state={"epoch": 0, "global_step": 17})
    a = torch.load(with_ema, map_location="cpu", weights_only=True)
    b = torch.load(without, map_location="cpu", weights_only=True)
    assert sorted(set(a) - set(b)) == ["ema_state_dict", "spdm_ema"] and list(b) == [k for k in a if k in b]
    assert "ema_state_dict" not in b and "spdm_ema" not in b
    assert a["spdm_ema"] == {"optimization_step": 17, "schedule": dict(EMA_SCHEDULE, max_value=0.999)}
    assert list(a["ema_state_dict"]) == list(a["state_dict"])
    for k, v in a["ema_state_dict"].items():
        assert v.device.type == "cpu" and v.dtype == torch.float32 and torch.equal(v, a["state_dict"][k] * 0.5), k
        assert torch.equal(a["state_dict"][k], b["state_dict"][k])

    hp = str(tmp_path / "hparams.yaml")
    m.save_hparams(hp)
    live = Diffusion_DDPM.load_from_checkpoint(with_ema, hparams_file=hp)
    avg = Diffusion_DDPM.load_from_checkpoint(with_ema, hparams_file=hp, use_ema=True)
    for k, v in m.noise_estimator._host_sd.items():
        assert np.array_equal(live.noise_estimator._sd[k], v) and np.array_equal(avg.noise_estimator._sd[k], v * np.float32(0.5)), k
    assert avg._ema is None                                                   # for inference: it holds weights, not an average
    with pytest.raises(ValueError, match="ema_state_dict"):
        Diffusion_DDPM.load_from_checkpoint(without, hparams_file=hp, use_ema=True)
    with pytest.raises(ValueError, match="ema_state_dict"):
        load_model("DDPM", without, hp, use_ema=True)
    with pytest.raises(ValueError, match="checkpoint"):
        load_model("DDPM", None, None, use_ema=True, **HP)
    assert np.array_equal(load_model("DDIM", with_ema, hp, use_ema=True).noise_estimator._sd["outc.weight"],
                          avg.noise_estimator._sd["outc.weight"])


def test_model_without_an_ema_refuses_to_use_one():
    m = Diffusion_DDPM(model="UNet_FilmnoAttention", weight_seed=5, **HP)
    with pytest.raises(RuntimeError, match="configure_ema"):
        with m.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="configure_ema"):
        m.validation_loss([], use_ema=True)
    with pytest.raises(RuntimeError, match="configure_ema"):
        m.sample({}, use_ema=True)
