"""A float64 numpy restatement of the reference's dataset (utils/load_data.py:11-143, utils/data_utils.py:10-62), written from
its description: the window table, the statistics, and one batch as the model sees it after its ``.float()`` casts.  Test
support only: the product path is state_policy_diffusionmodel_amd/dataset.py and csrc/dataset.hip, compared against this."""
import numpy as np


def window_table(ends, seq, step):
    rows, prev = [], 0
    for end in ends:
        for start in range(prev, int(end) - seq + 1):
            if start + seq * step <= end:
                rows.append([start, start + seq * step, 0, seq])
        prev = int(end)
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


def column_stats(x):
    x = x.reshape(-1, x.shape[-1])
    return {"min": x.min(axis=0), "max": x.max(axis=0)}


def normalize(x, st):
    return (x - st["min"]) / (st["max"] - st["min"]) * 2 - 1


def stats(position, velocity, action, table, step):
    mins, maxs = [], []
    for start, end, _, _ in table:
        w = position[start:end:step]
        mins.append(w.min(axis=0))
        maxs.append(w.max(axis=0))
    return {"position": {"max": np.average(maxs), "min": np.average(mins)}, "velocity": column_stats(velocity),
            "action": column_stats(action)}


def window(position, nvelocity, naction, table, step, i, pos_stats):
    """Window i: (position (seq,2), translation (2,), velocity (seq,2), action (seq,3)), float64."""
    start, end = int(table[i, 0]), int(table[i, 1])
    sn = normalize(position[start:end:step], pos_stats)
    tr = sn[0, :]
    return (sn - tr) / 2.0, tr, nvelocity[start:end:step], naction[start:end:step]


def frames_f32(img, rows):
    """Store rows of ``img`` (T,96,96,3) as the model gets them: (n,3,96,96) float32."""
    return np.moveaxis(img[np.asarray(rows)], -1, 1).astype(np.float32)


def batch(position, velocity, action, img, ends, obs, pred, step, ids, n_frames, st=None):
    """The batch of windows ``ids``: float32 'image' (B,n_frames,3,96,96; absent for n_frames = 0), 'position', 'velocity',
    'action', and float64 'translation', int 'start' / 'end'.  Float64 arithmetic, rounded once to float32."""
    seq = obs + pred
    table = window_table(ends, seq, step)
    st = st or stats(position, velocity, action, table, step)
    nvel, nact = normalize(velocity, st["velocity"]), normalize(action, st["action"])
    out = {k: [] for k in ("position", "translation", "velocity", "action", "start", "end", "image")}
    for i in ids:
        p, tr, v, a = window(position, nvel, nact, table, step, i, st["position"])
        start, end = int(table[i, 0]), int(table[i, 1])
        out["position"].append(p.astype(np.float32))
        out["velocity"].append(v.astype(np.float32))
        out["action"].append(a.astype(np.float32))
        out["translation"].append(tr)
        out["start"].append(start)
        out["end"].append(end)
        out["image"].append(frames_f32(img, np.arange(start, end, step)[:n_frames]))
    res = {k: np.stack(v) for k, v in out.items()}
    if n_frames == 0:
        del res["image"]
    return res
