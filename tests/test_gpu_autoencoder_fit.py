"""The autoencoder's run on the GPU: spdm_recon_terms and spdm_frames_to_bytes against their numpy restatements
bit for bit, validation_loss as a deterministic function of weights and frames, train.fit's files, an exact resume, the
checkpoint chain into the diffusion model, and the reconstruction report.  40 structured frames, 32 train / 8 validation,
batches of 8, two epochs."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import frames_u8_ref
import loss_terms_ref
import recon_terms_ref
from autoencoder_fit_ref import restate_run, structured_frames

pytestmark = pytest.mark.gpu

SEED, WEIGHT_SEED, BATCH = 7, 3, 8
FRAME = recon_terms_ref.FRAME
# |final val_loss of tests/autoencoder_fit_ref.restate_run in float32 - the same in float64| on the CPU, for this data, seed
# and initialisation: 0.04249671526165747 against 0.042496715029427604.  The run may differ from the float64 restatement by
# four times that: its kernels are exact fp32 with summation orders of their own.
F32_F64_GAP = 2.33e-10


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.int32)


def _same_state(a, b, what):
    """two optimiser / model states: every tensor bit for bit, every number equal"""
    assert type(a) is type(b), what
    if isinstance(a, dict):
        assert list(a.keys()) == list(b.keys()), what
        for k in a:
            _same_state(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_state(x, y, f"{what}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.float()), _bits(b.float())), what
    else:
        assert a == b or (a != a and b != b), (what, a, b)


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint64 if got.dtype == np.float64 else np.uint8), want.view(np.uint64 if want.dtype == np.float64 else np.uint8)), what


# ---- spdm_recon_terms ------------------------------------------------------------------------------------------------------------
def _term_cases():
    """name -> (recon, target), 5 frames each (7 for the single errors)"""
    rng = np.random.default_rng(21)
    uni = (rng.random((5, 3, 96, 96), dtype=np.float32), rng.random((5, 3, 96, 96), dtype=np.float32))
    same = (uni[1].copy(), uni[1].copy())
    spots = (0, 3, 4, 1023, 1024, 27644, 27647)
    target = rng.random((len(spots), FRAME), dtype=np.float32)
    recon = target.copy()
    for f, e in enumerate(spots):                                       # a dropped head, tail or quad boundary loses the frame's one error
        recon[f, e] += np.float32(0.25 + 0.01 * f)
    single = (recon.reshape(-1, 3, 96, 96), target.reshape(-1, 3, 96, 96))
    t = rng.random((5, FRAME), dtype=np.float32)
    r = t.copy()
    r[:, 0::2] += np.float32(1e-4)                                       # errors of 1e-4 and of 1 interleaved: the order shows in float64
    r[:, 1::2] -= np.float32(1.0)
    mixed = (r.reshape(-1, 3, 96, 96), t.reshape(-1, 3, 96, 96))
    return {"uniform": uni, "identical": same, "single": single, "mixed": mixed}


@pytest.mark.parametrize("slot_offset", [0, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_recon_terms_match_the_restatement_bit_for_bit(n, slot_offset):
    from state_policy_diffusionmodel_amd.train_metrics import recon_terms_into
    for name, (recon, target) in _term_cases().items():
        k = recon.shape[0] if name == "single" else n
        recon, target = recon[:k], target[:k]
        terms = torch.full((slot_offset + k + 2,), -7.0, dtype=torch.float64, device="cuda")
        recon_terms_into(torch.from_numpy(recon).cuda(), torch.from_numpy(target).cuda(), terms, slot_offset)
        got = terms.cpu().numpy()
        want = recon_terms_ref.recon_terms(recon, target)
        same_bits(got[slot_offset:slot_offset + k], want, name)
        assert (got[:slot_offset] == -7.0).all() and (got[slot_offset + k:] == -7.0).all(), name      # sentinel slots untouched
        if name == "identical":
            assert not got[slot_offset:slot_offset + k].any()           # exactly 0.0
        if name == "single":
            assert (want > 0).all()


def test_recon_terms_nan_stays_in_its_frame():
    from state_policy_diffusionmodel_amd.train_metrics import recon_terms_into
    recon, target = (a[:3].copy() for a in _term_cases()["uniform"])
    recon[1, 2, 50, 17] = np.nan
    terms = torch.zeros(3, dtype=torch.float64, device="cuda")
    recon_terms_into(torch.from_numpy(recon).cuda(), torch.from_numpy(target).cuda(), terms)
    got, want = terms.cpu().numpy(), recon_terms_ref.recon_terms(recon, target)
    assert np.isnan(got).tolist() == [False, True, False] == np.isnan(want).tolist()
    same_bits(got[[0, 2]], want[[0, 2]], "the frames beside the NaN")


# ---- spdm_frames_to_bytes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_offset", [0, 2])
@pytest.mark.parametrize("cols", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_frames_to_u8_matches_the_restatement_bit_for_bit(n, cols, tile_offset):
    from state_policy_diffusionmodel_amd.dataset import frames_to_u8
    x = frames_u8_ref.edge_frames(n, seed=n)
    n_tiles = tile_offset + n + 1                                        # one tile after the last stays untouched too
    held = np.full(frames_u8_ref.sheet_shape(n_tiles, cols), 0xA5, np.uint8)
    out = torch.from_numpy(held).cuda()
    back = frames_to_u8(torch.from_numpy(x).cuda(), out, cols=cols, tile_offset=tile_offset, n_tiles=n_tiles)
    assert back is out
    want = frames_u8_ref.frames_to_u8(x, cols, tile_offset, n_tiles, out=held)
    same_bits(out.cpu().numpy(), want, "sheet")
    assert (want == 0xA5).sum() >= (n_tiles - n) * 96 * 96 * 3          # the restatement left the other tiles alone, so the kernel did


def test_gather_then_frames_to_u8_is_the_identity():
    from state_policy_diffusionmodel_amd.dataset import FrameStore, frames_to_u8
    img = np.random.default_rng(3).integers(0, 256, (6, 96, 96, 3), dtype=np.uint8)
    img[0, 0, :, 0] = np.arange(96) * 2                                  # every byte value occurs
    img[0, 1, :, 1] = np.arange(96) * 2 + 1
    img[0, 2, :64, 2] = np.arange(192, 256)
    store = FrameStore(img)
    assert store.image_storage == "uint8" and len(store) == 6
    ids = [4, 0, 5, 0, 2]
    frames = store.frames(ids)
    assert frames.shape == (5, 3, 96, 96) and store.last_bad() == 0
    sheet = frames_to_u8(frames, cols=1)
    assert sheet.shape == (5 * 96, 96, 3)
    assert np.array_equal(sheet.cpu().numpy().reshape(5, 96, 96, 3), img[ids])
    as_float = FrameStore(img.astype(np.float32) / np.float32(255), image_storage="float32")
    assert torch.equal(as_float.frames(ids), frames)


# ---- the run -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data():
    from state_policy_diffusionmodel_amd.dataset import FramesDataModule
    dm = FramesDataModule(BATCH, seed=SEED)
    dm.setup(arrays={"img": structured_frames()})
    assert len(dm.data_full) == 40 and len(dm.train_ids) == 32 and len(dm.val_ids) == 8 and dm.data_full.image_storage == "uint8"
    return dm


def _model():
    from state_policy_diffusionmodel_amd.autoencoder import autoencoder
    return autoencoder(learning_rate=1e-3, weight_seed=WEIGHT_SEED)


def _fit(model, out, epochs, **kw):
    from state_policy_diffusionmodel_amd.train import fit
    # train_autoencoder's settings but for the early stop: its patience of n_epochs VALIDATIONS would end a 2-epoch run at the third
    return fit(model, _data(), max_epochs=epochs, out_dir=out, val_check_interval=0.5, gradient_clip_val=0.5, seed=SEED,
               early_stop=None, validate_first=True, device_optimizer=True, **kw)


@functools.lru_cache(maxsize=None)
def _one_go(tmp):
    model = _model()
    initial = model.state_dict()
    return model, initial, _fit(model, tmp, 2)


@pytest.fixture(scope="module")
def one_go(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("ae_one_go"))
    return (tmp,) + _one_go(tmp)


def test_two_constructions_with_one_seed_are_bit_equal():
    a, b = _model().state_dict(), _model().state_dict()
    _same_state(a, b, "state_dict")
    assert _model().model_name == "autoencoder"
    with pytest.raises(TypeError):
        _model().training_step(torch.zeros(1, 3, 96, 96), t=None)


def test_validation_loss_is_the_restated_mean_of_the_restated_terms():
    from state_policy_diffusionmodel_amd.dataset import _FrameBatches
    model, dm = _model(), _data()
    val_loss, terms = model.validation_loss(dm.val_dataloader(), seed=SEED, return_terms=True)
    x = dm.data_full.frames(dm.val_ids)
    recon = model.decoder(model.encoder(x))
    want = recon_terms_ref.recon_terms(recon.cpu().numpy(), x.cpu().numpy())
    assert terms.shape == (8,) and terms.dtype == torch.float64 and terms.is_cuda
    same_bits(terms.cpu().numpy(), want, "terms")
    assert isinstance(val_loss, float) and val_loss == float(loss_terms_ref.pass_mean(want))      # spdm_eval_reduce's order, restated
    exact = math.fsum(want.tolist()) / 8
    assert abs(val_loss - exact) <= 8 * 2.0 ** -53 * exact

    again, terms2 = model.validation_loss(dm.val_dataloader(), return_terms=True)
    assert again == val_loss and torch.equal(terms, terms2) and model.validation_loss(dm.val_dataloader()) == val_loss
    at3, terms3 = model.validation_loss(_FrameBatches(dm.data_full, dm.val_ids, 3), return_terms=True)
    assert at3 == val_loss and torch.equal(terms3, terms)                # the batch size changes nothing

    # one batch: float32(val_loss) against training_step's device loss, two float32 roundings of float64 sums of the same squares
    loss = float(model.training_step(x).item())
    as32 = float(np.float32(val_loss))
    ulp = float(np.spacing(np.float32(as32)))
    print(f"val_loss {val_loss!r} as fp32 {as32!r}; training_step {loss!r}; ulp {ulp:.3e}")
    assert abs(as32 - loss) <= ulp


def test_fit_writes_what_a_training_run_leaves_behind(one_go):
    out, model, initial, res = one_go
    assert sorted(os.listdir(os.path.join(out, "checkpoints"))) == ["epoch=0.ckpt", "epoch=1.ckpt"]
    assert sorted(f for f in os.listdir(out) if f != "checkpoints") == ["hparams.yaml", "metrics.jsonl"]      # no STATS.pkl
    assert open(os.path.join(out, "hparams.yaml")).read().strip() == "learning_rate: 0.001"
    lines = [json.loads(x) for x in open(os.path.join(out, "metrics.jsonl"))]
    assert lines == res["metrics"]
    # 4 train batches an epoch: a validation after the 2nd and the 4th (int(4 * 0.5) = 2); one before training; one line per epoch end
    assert [(x["kind"], x["epoch"], x["global_step"]) for x in lines] == [
        ("val", -1, 0), ("val", 0, 2), ("val", 0, 4), ("epoch", 0, 4), ("val", 1, 6), ("val", 1, 8), ("epoch", 1, 8)]
    assert all(math.isfinite(x["val_loss"]) and x["val_loss"] > 0 for x in lines)
    assert res["global_step"] == 8 and res["epoch"] == 1 and not res["stopped_early"]
    for e in (0, 1):
        raw = torch.load(os.path.join(out, "checkpoints", f"epoch={e}.ckpt"), map_location="cpu", weights_only=True)
        assert raw["epoch"] == e and raw["global_step"] == 4 * (e + 1) and raw["hyper_parameters"] == {"learning_rate": 1e-3}
        assert float(raw["optimizer_states"][0]["state"][0]["step"]) == 4.0 * (e + 1)
        assert sorted(k.split(".")[0] for k in raw["state_dict"]) == ["decoder"] * 8 + ["encoder"] * 8 + ["model"] * 16
    _same_state(raw["state_dict"], model.state_dict(), "the last checkpoint holds the trained weights")
    assert not torch.equal(raw["state_dict"]["decoder.6.weight"], initial["decoder.6.weight"])
    assert res["val_loss"] == model.validation_loss(_data().val_dataloader())


def test_the_run_learns_and_agrees_with_the_float64_restatement(one_go):
    from state_policy_diffusionmodel_amd.dataset import _epoch_order
    out, model, initial, res = one_go
    dm = _data()
    orders = [dm.train_ids[_epoch_order(len(dm.train_ids), SEED, e)] for e in range(2)]
    assert [o.tolist() for o in orders] == [dm.train_dataloader(e).row_ids.tolist() for e in range(2)]
    first64, last64 = restate_run(initial, structured_frames(), orders, dm.val_ids, batch_size=BATCH, dtype=torch.float64)
    first, last = res["metrics"][0]["val_loss"], res["val_loss"]
    print(f"validate-first {first!r} (float64 restatement {first64!r}); final {last!r} (float64 restatement {last64!r}); "
          f"|diff| {abs(last - last64):.3e}, allowed {4 * F32_F64_GAP:.3e}")
    assert last64 < first64                                              # the restatement itself shows the decrease
    assert last < first
    assert abs(last - last64) <= 4 * F32_F64_GAP


def test_resume_is_exact(one_go, tmp_path):
    from state_policy_diffusionmodel_amd.autoencoder import autoencoder
    out, model, initial, res = one_go
    _fit(_model(), tmp_path, 1)
    ckpt0 = os.path.join(str(tmp_path), "checkpoints", "epoch=0.ckpt")
    fresh = autoencoder.load_from_checkpoint(ckpt0)
    res2 = _fit(fresh, tmp_path, 2, ckpt_path=ckpt0)
    a = [json.loads(x) for x in open(os.path.join(out, "metrics.jsonl"))]
    b = [json.loads(x) for x in open(os.path.join(str(tmp_path), "metrics.jsonl"))]
    assert a == b                                                        # every val_loss, every logged train loss, every lr
    assert {k: v for k, v in res2.items() if k != "metrics"} == {k: v for k, v in res.items() if k != "metrics"}
    one = torch.load(os.path.join(out, "checkpoints", "epoch=1.ckpt"), map_location="cpu", weights_only=True)
    two = torch.load(os.path.join(str(tmp_path), "checkpoints", "epoch=1.ckpt"), map_location="cpu", weights_only=True)
    _same_state(one, two, "checkpoint")                                  # both halves' weights, Adam state, scheduler, counters
    for half in ("encoder", "decoder"):
        assert torch.equal(_bits(getattr(fresh, half).flat_parameter()), _bits(getattr(model, half).flat_parameter())), half
    # restore_checkpoint wrote in place: a second model restored from the dict keeps its parameters' addresses
    other = _model()
    params = other._params()
    ptrs = [p.data_ptr() for p in params]
    other.restore_checkpoint(one)
    assert [p.data_ptr() for p in other._params()] == ptrs and other._params()[0] is params[0]
    _same_state(other.state_dict(), one["state_dict"], "restored")
    assert other.validation_loss(_data().val_dataloader()) == res["val_loss"]


def test_the_checkpoint_feeds_the_diffusion_model(one_go, tmp_path):
    import test_gpu_fit as diffusion_fit
    from state_policy_diffusionmodel_amd import train
    from state_policy_diffusionmodel_amd.autoencoder import autoencoder
    from state_policy_diffusionmodel_amd.diffusion import Diffusion_DDPM
    from state_policy_diffusionmodel_amd.weights import safe_load_state_dict
    out, model, initial, res = one_go
    ckpt = os.path.join(out, "checkpoints", "epoch=1.ckpt")
    x = _data().data_full.frames(_data().val_ids)
    want = model.encoder(x)
    assert not torch.equal(want, autoencoder(state_dict=initial).encoder(x))                    # the trained encoder, not the initial one
    assert torch.equal(autoencoder.load_from_checkpoint(ckpt).encoder(x), want)
    ddpm = Diffusion_DDPM(noise_steps=20, obs_horizon=2, pred_horizon=4, observation_dim=135, prediction_dim=5,
                          model="UNet_FilmnoAttention", inpaint_horizon=2, step_size=5, weight_seed=3, max_batch=8,
                          vision_encoder_state_dict=safe_load_state_dict(ckpt))
    enc_sd = {k: v for k, v in model.encoder.state_dict().items()}
    assert torch.equal(ddpm._trainable_encoder()(x), want)               # the model's own VisionEncoder, built from those tensors

    arrays = diffusion_fit._arrays()
    npz = str(tmp_path / "windows.npz")
    np.savez(npz, **arrays)
    run = str(tmp_path / "run")
    r = train.main(["--arrays", npz, "--encoder_checkpoint", ckpt, "--n_epochs", "1", "--batch_size", "8", "--obs_horizon", "2",
                    "--pred_horizon", "4", "--inpaint_horizon", "2", "--noise_steps", "20", "--model", "UNet_FilmnoAttention",
                    "--out_dir", run, "--no_early_stop"])
    assert r["epoch"] == 0 and math.isfinite(r["val_loss"])
    raw = torch.load(os.path.join(run, "checkpoints", "epoch=0.ckpt"), map_location="cpu", weights_only=True)
    for k, v in enc_sd.items():                                          # the diffusion run's checkpoint carries the trained encoder
        assert torch.equal(_bits(raw["state_dict"]["vision_encoder." + k]), _bits(v)), k
    from state_policy_diffusionmodel_amd.vision import VisionEncoder, encoder_state_dict_from
    assert torch.equal(VisionEncoder(encoder_state_dict_from(raw["state_dict"]))(x), want)


def test_reconstruction_report_and_the_eval_command(one_go, tmp_path):
    from state_policy_diffusionmodel_amd import eval_autoencoder
    out, model, initial, res = one_go
    dm = _data()
    rep = model.reconstruction_report(dm.val_dataloader(), sheet_frames=5, cols=3)
    val_loss, terms = model.validation_loss(dm.val_dataloader(), return_terms=True)
    assert rep["val_loss"] == val_loss == res["val_loss"]
    mse = terms.cpu().numpy()
    same_bits(rep["terms"], mse, "terms")
    psnr = 10.0 * np.log10(1.0 / mse)
    assert rep["psnr_mean"] == float(psnr.mean()) and rep["psnr_min"] == float(psnr.min())
    assert rep["worst"] == [int(dm.val_ids[i]) for i in np.argsort(-mse, kind="stable")[:5]]
    x = dm.data_full.frames(dm.val_ids[:5])
    recon = model.decoder(model.encoder(x))
    want = np.zeros(frames_u8_ref.sheet_shape(12, 3), np.uint8)          # 2 rows of originals (5 of 6 tiles), 2 rows of reconstructions
    want = frames_u8_ref.frames_to_u8(x.cpu().numpy(), 3, 0, 12, out=want)
    want = frames_u8_ref.frames_to_u8(recon.cpu().numpy(), 3, 6, 12, out=want)
    sheet = rep["sheet"]
    assert sheet.is_cuda and sheet.dtype == torch.uint8 and sheet.shape == (4 * 96, 3 * 96, 3)
    same_bits(sheet.cpu().numpy(), want, "sheet")
    assert np.array_equal(want[:96, :96], structured_frames()[dm.val_ids[0]])                  # the originals are the stored bytes

    npz, js, ppm = str(tmp_path / "frames.npz"), str(tmp_path / "report.json"), str(tmp_path / "sheet.ppm")
    np.savez(npz, img=structured_frames())
    got = eval_autoencoder.main(["--checkpoint", os.path.join(out, "checkpoints", "epoch=1.ckpt"), "--arrays", npz, "--seed", str(SEED),
                                 "--batch_size", "8", "--out", js, "--sheet", ppm, "--sheet_frames", "5", "--columns", "3", "--terms"])
    report = json.load(open(js))
    assert report["val_loss"] == val_loss and report["frames"] == 8 and report["terms"] == mse.tolist() and report["worst"] == rep["worst"]
    assert got["val_loss"] == val_loss
    raw = open(ppm, "rb").read()
    head = b"P6\n288 384\n255\n"
    assert raw[:len(head)] == head and raw[len(head):] == want.tobytes()
