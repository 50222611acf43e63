"""tests/frames_u8_ref.py (the restatement of spdm_frames_to_bytes) against what it must satisfy on its own -- the identity on
the bytes the gather emits, the tiling, untouched tiles -- and against the mutants it could be confused with."""
import numpy as np
import pytest

import frames_u8_ref


def test_every_byte_round_trips():
    k = np.arange(256, dtype=np.float32)
    x = k / np.float32(255)                                              # what spdm_dataset_gather emits for a stored byte
    assert np.array_equal((x * np.float32(255)), k)                      # v == k exactly: nothing is left to round
    assert np.array_equal(frames_u8_ref.quantise(x), np.arange(256, dtype=np.uint8))


def test_specials_and_ties():
    q = frames_u8_ref.quantise
    x = np.array([-0.0, -1.0, -np.inf, np.nan, np.inf, 2.0, 1.0], np.float32)
    assert q(x).tolist() == [0, 0, 0, 0, 255, 255, 255]
    half = np.array([0.5, 1.5, 2.5, 127.5, 254.5], np.float32) / np.float32(255)
    exact = half[(half * np.float32(255)) == np.array([0.5, 1.5, 2.5, 127.5, 254.5], np.float32)]
    assert exact.size                                                    # some products are exact ties: they go to the even byte
    assert (q(exact) % 2 == 0).all()


def test_cols_one_is_the_stores_layout_and_other_tiles_are_kept():
    x = frames_u8_ref.edge_frames(3, seed=2)
    sheet = frames_u8_ref.frames_to_u8(x)
    assert sheet.shape == (3 * 96, 96, 3)
    assert np.array_equal(sheet.reshape(3, 96, 96, 3), frames_u8_ref.quantise(x).transpose(0, 2, 3, 1))
    held = np.full(frames_u8_ref.sheet_shape(7, 3), 0xA5, np.uint8)
    out = frames_u8_ref.frames_to_u8(x, cols=3, tile_offset=2, n_tiles=7, out=held)
    assert np.array_equal(out[0:96, 192:288], sheet[0:96])               # tile 2: row 0, column 2
    assert np.array_equal(out[96:192, 0:96], sheet[96:192]) and np.array_equal(out[96:192, 96:192], sheet[192:288])
    untouched = out.copy()
    untouched[0:96, 192:288] = 0xA5
    untouched[96:192, 0:192] = 0xA5
    assert (untouched == 0xA5).all()


@pytest.mark.parametrize("name,knobs", [("fp64 multiply", {"mul": np.float64}), ("floor(v + 0.5)", {"floor_half": True}),
                                         ("x / y swapped", {"swap_xy": True}), ("channel order reversed", {"reverse_channels": True}),
                                         ("tile row / column swapped", {"swap_tile": True})])
def test_mutants_of_the_restatement_show(name, knobs):
    x = frames_u8_ref.edge_frames(5, seed=1)
    true = frames_u8_ref.frames_to_u8(x, cols=3, tile_offset=2, n_tiles=9)
    mutant = frames_u8_ref.frames_to_u8(x, cols=3, tile_offset=2, n_tiles=9, **knobs)
    assert not np.array_equal(true, mutant), name
