"""tests/policy_ref.py against tests/golden/policy_small.npz, which tools/make_golden_policy.py recorded from the reference's own
utils/data_utils.py functions driven as run_predictions.py drives them (deques, list(...)[::s], torch.tensor(..., float32)):
bit for bit.  And the row arithmetic of the replay CLI against the dataset's window table.  No GPU."""
import os

import numpy as np

import dataset_ref
import policy_ref
from state_policy_diffusionmodel_amd.run_predictions import plan_rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load():
    return np.load(os.path.join(GOLDEN, "policy_small.npz")), np.load(os.path.join(GOLDEN, "dataset_small.npz"))


def _stats(d, dt):
    return {"position": {"min": d["s5/pos_min"][()], "max": d["s5/pos_max"][()]},
            "velocity": {k: d["s5/vel_" + k].astype(dt) for k in ("min", "max")},
            "action": {k: d["s5/act_" + k].astype(dt) for k in ("min", "max")}}


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = np.count_nonzero(got.view(bits) != want.view(bits))
    assert diff == 0, f"{what}: {diff} of {got.size} elements differ"


def test_the_restatement_equals_the_recorded_reference_bit_for_bit():
    g, d = _load()
    seen = set()
    for i in range(int(g["n_cases"])):
        c = f"c{i}/"
        obs_h, s, first, pushes = (int(g[c + k]) for k in ("obs_h", "step_size", "first", "pushes"))
        resets, dt = g[c + "resets"].tolist(), str(g[c + "stats_dtype"])
        stats = _stats(d, dt)
        L = obs_h * s
        h = policy_ref.History(1, L)
        img = np.zeros((1, 96, 96, 3), np.uint8)                                # frames are not part of the recording
        for n in range(pushes):
            if n in resets and n > 0:
                h.reset()
            r = first + n
            h.push(img, d["position"][r:r + 1], d["velocity"][r:r + 1], d["action"][r:r + 1])
            b = policy_ref.batch(h, stats, s)
            for k in ("position", "velocity", "action", "translation"):
                same_bits(b[k][0], g[c + k][n], (i, n, k))
        seen.add((dt, pushes > 2 * L, len(resets) > 1))
    # both statistics dtypes, a history that has wrapped, a reset mid-stream
    assert {x[0] for x in seen} == {"float64", "float32"} and any(x[1] for x in seen) and any(x[2] for x in seen)


def test_a_reset_refills_only_the_environments_named():
    h = policy_ref.History(3, 4)
    rng = np.random.default_rng(0)
    obs = [(np.full((3, 96, 96, 3), n, np.uint8), rng.standard_normal((3, 2)), rng.standard_normal((3, 2)), rng.standard_normal((3, 3)))
           for n in range(7)]
    for n in range(7):
        if n == 5:
            h.reset([1])
        h.push(*obs[n])
    w = h.window(1)
    assert w["image"][:, :, 0, 0, 0].tolist() == [[3, 4, 5, 6], [5, 5, 5, 6], [3, 4, 5, 6]]
    assert np.array_equal(w["position"][1, 0], obs[5][1][1].astype(np.float32))
    assert h.window(2)["image"][:, :, 0, 0, 0].tolist() == [[3, 5], [5, 5], [3, 5]]


def test_plan_rows_are_the_rows_of_the_dataset_window_that_starts_l_minus_one_rows_earlier():
    _, d = _load()
    ends = d["episode_ends"].tolist()
    for obs_h, pred, s in ((2, 4, 5), (2, 4, 1), (3, 2, 2)):
        table = dataset_ref.window_table(ends, obs_h + pred, s)
        assert np.array_equal(table, d[f"s{s}/indices"]) if (obs_h, pred) == (2, 4) and s in (1, 5) else len(table) > 0
        L = obs_h * s
        for start, stop, _, _ in table.tolist():
            end = min(e for e in ends if e > start)
            first = max([0] + [e for e in ends if e <= start])
            observed, predicted, left_out = plan_rows(start + L - 1, first, end, obs_h, pred, s)
            assert observed + predicted == list(range(start, stop, s)) and left_out == 0, (start, s)


def test_plan_rows_at_the_edges_of_an_episode():
    # the history still holds the initial fill: rows before the episode's first are the first
    assert plan_rows(61, 61, 140, 4, 3, 5) == ([61, 61, 61, 61], [62, 67, 72], 0)
    assert plan_rows(70, 61, 140, 4, 3, 5) == ([61, 61, 61, 66], [71, 76, 81], 0)
    # way-points past the episode's end are left out and counted
    assert plan_rows(130, 61, 140, 2, 4, 5) == ([121, 126], [131, 136], 2)
    assert plan_rows(139, 61, 140, 2, 4, 5) == ([130, 135], [], 4)
    for bad in (60, 140):
        try:
            plan_rows(bad, 61, 140, 2, 4, 5)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_u_agrees_with_the_reference_on_float32_inputs_within_its_float32_roundings():
    """The reference's unnormalize_position on float32 arrays (run_predictions.py:159-164) computes
        s32 = fl32(2 n + tr)          one float32 rounding (2 n is exact):  |s32 - s|        <= 2^-24 |s|
        h32 = fl32(s32 + 1) / 2       one more (the halving is exact):      |2 h32 - (s32+1)| <= 2^-24 |s32 + 1|
    and only then widens: h32 * (max - min) + min in float64.  U forms s + 1 in float64, where it is exact to 2^-53.  So
    |(2 h32) - (s + 1)| <= 2^-24 |s| + 2^-24 (|s| (1 + 2^-24) + 1) < 2^-23 (|s| + 1), and after the halving and the scaling the
    two differ by less than 2^-24 (|s| + 1) (max - min) plus a few float64 roundings of a value of size (|s| + 1) (max - min) / 2.
    The bound asserted is twice the float32 part, 2^-23 (max|s| + 1) (max - min), which leaves the float64 part (2^-52 relative)
    far below the slack."""
    g, d = _load()
    pos_min, pos_max = d["s5/pos_min"][()], d["s5/pos_max"][()]
    pred, tr, want = g["un/pred"], g["un/translation"], g["un/out"]
    assert pred.dtype == tr.dtype == np.float32 and want.dtype == np.float64
    got = policy_ref.U(pred, tr, pos_min, pos_max)
    sn = pred.astype(np.float64) * 2.0 + tr.astype(np.float64)[:, None, :]
    bound = 2.0 ** -23 * (np.abs(sn).max() + 1.0) * (pos_max - pos_min)
    diff = np.abs(got - want).max()
    print(f"max |U - unnormalize_position| = {diff:.3e}, bound {bound:.3e}")
    assert 0 < diff <= bound
