"""dataset.py's numpy helpers and tests/dataset_ref.py against values recorded from the reference's own functions
(tests/golden/dataset_small.npz, tools/make_golden_dataset.py), exactly: integer tables and float64 results of the same
IEEE operations.  Plus the split, the uint8 rule and the storage decision.  No GPU."""
import os

import numpy as np
import pytest
import torch

import dataset_ref
from state_policy_diffusionmodel_amd import dataset as ds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_small.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("step,n", [(5, 58), (1, 124)])
def test_tables_stats_and_every_window_equal_the_recording(gold, step, n):
    pos, vel, act, ends, seq = gold["position"], gold["velocity"], gold["action"], gold["episode_ends"], int(gold["sequence_length"])
    k = f"s{step}/"
    want = gold[k + "indices"]
    assert want.shape == (n, 4) and want[-1, 1] == 140          # the last window ends exactly at the last row
    for table in (ds.create_sample_indices_sparse(ends, seq, step), dataset_ref.window_table(ends, seq, step)):
        assert table.dtype == np.int64 and np.array_equal(table, want)
    for st in (ds.compute_stats(pos, vel, act, want, step), dataset_ref.stats(pos, vel, act, want, step)):
        assert st["position"]["min"] == gold[k + "pos_min"] and st["position"]["max"] == gold[k + "pos_max"]
        assert np.ndim(st["position"]["min"]) == 0
        assert np.array_equal(st["velocity"]["min"], gold[k + "vel_min"]) and np.array_equal(st["velocity"]["max"], gold[k + "vel_max"])
        assert np.array_equal(st["action"]["min"], gold[k + "act_min"]) and np.array_equal(st["action"]["max"], gold[k + "act_max"])
    st = ds.compute_stats(pos, vel, act, want, step)
    nvel, nact = ds.normalize_data(vel, st["velocity"]), ds.normalize_data(act, st["action"])
    assert nvel.dtype == np.float64
    for i in range(n):
        p, tr, v, a = dataset_ref.window(pos, nvel, nact, want, step, i, st["position"])
        assert np.array_equal(p, gold[k + "position"][i]) and np.array_equal(tr, gold[k + "translation"][i])
        assert np.array_equal(v, gold[k + "velocity"][i]) and np.array_equal(a, gold[k + "action"][i])
    # dataset_ref.batch is those windows rounded once to float32
    ids = [0, n - 1, 7, 7]
    got = dataset_ref.batch(pos, vel, act, np.zeros((140, 96, 96, 3), np.float32), ends, 2, seq - 2, step, ids, 0)
    assert "image" not in got and got["position"].dtype == np.float32
    assert np.array_equal(got["position"], gold[k + "position"][ids].astype(np.float32))
    assert np.array_equal(got["action"], gold[k + "action"][ids].astype(np.float32))
    assert np.array_equal(got["translation"], gold[k + "translation"][ids])
    assert np.array_equal(got["start"], want[ids, 0]) and np.array_equal(got["end"], want[ids, 1])
    # and the (un)normalisation pair round-trips
    assert np.allclose(ds.unnormalize_data(nvel, st["velocity"]), vel, rtol=0, atol=1e-12)


def test_short_episodes_contribute_no_window(gold):
    t5 = gold["s5/indices"]
    assert not ((t5[:, 0] >= 37) & (t5[:, 0] < 61)).any()          # the 23-row and the 1-row episode: 6 * 5 rows do not fit
    assert ds.create_sample_indices_sparse([3], 6, 1).shape == (0, 4)


@pytest.mark.parametrize("n,seed", [(58, 7), (124, 123), (10, 1)])
def test_split_is_random_split(n, seed):
    n_train = int(n * 0.8)
    tr, va = torch.utils.data.random_split(range(n), [n_train, n - n_train], generator=torch.Generator().manual_seed(seed))
    a, b = ds.split_indices(n, seed)
    assert list(a) == list(tr.indices) and list(b) == list(va.indices)
    torch.manual_seed(99)                                           # seed falsy: the default generator, as the reference
    tr, va = torch.utils.data.random_split(range(n), [n_train, n - n_train])
    torch.manual_seed(99)
    a, b = ds.split_indices(n, None)
    assert list(a) == list(tr.indices) and list(b) == list(va.indices)


def test_uint8_rule_holds_for_every_byte():
    k = np.arange(256)
    v = k / 255.0                                                   # what the data generators store, float64
    assert np.array_equal(np.rint(v * 255), k)
    assert np.array_equal(k.astype(np.float32) / np.float32(255), v.astype(np.float32))
    # a multiply by the reciprocal is NOT the same function
    assert (k.astype(np.float32) * np.float32(1 / 255) != v.astype(np.float32)).sum() > 0
    img = np.zeros((2, 96, 96, 3))
    img.reshape(-1)[:256 * 3] = np.repeat(v, 3)
    assert ds.choose_image_storage(img) == "uint8"
    assert ds.choose_image_storage(img.astype(np.float32)) == "uint8"
    assert ds.choose_image_storage(img, "float32") == "float32"


def test_auto_picks_float32_for_one_value_off_the_grid():
    img = (np.random.default_rng(0).integers(0, 256, (5, 96, 96, 3)) / 255.0)
    assert ds.choose_image_storage(img, chunk_rows=2) == "uint8"
    img[4, 95, 95, 2] = 0.5                                         # 127.5 / 255: between two bytes, in the LAST chunk
    assert ds.choose_image_storage(img, chunk_rows=2) == "float32"
    with pytest.raises(ValueError, match="uint8"):
        ds.choose_image_storage(img, "uint8", chunk_rows=2)
    for bad in (1.0 + 1 / 255, -1 / 255, np.nan):
        img[4, 95, 95, 2] = bad
        assert ds.choose_image_storage(img, chunk_rows=2) == "float32", bad
    with pytest.raises(ValueError, match="image_storage"):
        ds.choose_image_storage(img, "fp16")


def test_data_module_without_zarr_names_the_package():
    dm = ds.CarRacingDataModule(4, data_dir="nowhere")
    try:
        import zarr  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="zarr"):
            dm.setup(name="x.zarr")
    with pytest.raises(ValueError, match="either"):
        dm.setup()
