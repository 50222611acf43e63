"""bench.py's multi-rank plumbing, rehearsed on CPU: `python bench.py --gpus 2` must start two ranks BY ITSELF
(gloo, stub engine: no kernels), report n_gpus = 2 with the strong-scaling workload (BASELINE config 4: one global
batch sharded over the ranks) as `value` and the weak figure beside it, and must refuse -- non-zero exit -- to report
a run whose world size differs from --gpus."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    return env


def test_gpus_2_launches_two_ranks_and_reports_strong_scaling():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--stub-engine", "--backend", "gloo", "--steps", "3",
                        "--warmup", "1", "--batch", "64", "--horizon", "16"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 3 and d["warmup"] == 1
    assert d["config"]["global_batch"] == 64 and d["config"]["per_gpu_batch"] == 32
    assert d["config"]["parallelism"] == "batch-shard x2"
    assert abs(d["value"] - 64 * 1000.0 / d["ms_per_step"]) <= 1e-6 * d["value"]
    w = d["weak_scaling"]
    assert w["global_batch"] == 128 and w["per_gpu_batch"] == 64 and w["value"] > 0
    assert "B=64" in d["metric"] and "horizon=16" in d["metric"]


def test_weak_headline_on_request():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--stub-engine", "--backend", "gloo", "--steps", "2",
                        "--warmup", "1", "--batch", "64", "--scaling", "weak"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["scaling"] == "weak" and d["config"]["global_batch"] == 128 and d["strong_scaling"]["global_batch"] == 64


def test_world_size_mismatch_is_an_error():
    env = _env()
    env.update({"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--stub-engine", "--backend", "gloo", "--steps", "2",
                        "--warmup", "1", "--batch", "8"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0
    assert "refusing" in r.stderr
    assert r.stdout.strip() == ""


def test_single_rank_stub_line():
    r = subprocess.run([sys.executable, BENCH, "--stub-engine", "--steps", "2", "--warmup", "1", "--batch", "8"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip())
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["config"]["global_batch"] == 8


def test_launcher_terminates_the_other_ranks_when_one_dies():
    """A rank that dies before the rendezvous must not leave rank 0 waiting for the backend's own timeout: the launcher
    polls every child, terminates the rest on the first failure and exits non-zero."""
    import time
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--stub-engine", "--backend", "gloo", "--steps", "2",
                        "--warmup", "1", "--batch", "8", "--stub-fail-rank", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "a rank failed" in r.stderr
    assert time.monotonic() - t0 < 60
    assert not [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("{")]     # never a line from a broken job


def test_dump_outputs_writes_what_the_timed_path_returns(tmp_path):
    """--dump-outputs DIR: the iterates of the last timed step as float32 DIR/iterates.npy.  The stub engine hands x_T back
    unchanged, so the file must be the seeded synthetic x_T -- the same on every run."""
    import numpy as np
    import torch
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--stub-engine", "--steps", "2", "--warmup", "1", "--batch", "8",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, cwd=ROOT, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip())["steps"] == 2
    assert sorted(os.listdir(d)) == ["iterates.npy"]
    a = np.load(d / "iterates.npy")
    assert a.dtype == np.float32 and a.shape == (8, 1, 32, 3)
    g = torch.Generator().manual_seed(1000)                    # bench.py inputs(): cond first, then x_T
    torch.randn(8, 1, 10, 135, generator=g)
    np.testing.assert_array_equal(a, torch.rand(8, 1, 32, 3, generator=g).numpy())


def test_steps_may_exceed_the_schedule_length():
    """--steps sets the number of timed steps even past --train-steps: the loop starts over from x_T."""
    r = subprocess.run([sys.executable, BENCH, "--stub-engine", "--steps", "7", "--warmup", "3", "--train-steps", "4",
                        "--batch", "8"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip())
    assert d["steps"] == 7 and d["warmup"] == 3
    assert abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) <= 1e-6 * d["value"]


def test_dump_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """Above the size cap the dump keeps a seeded sample of whole rows, in order, identical from run to run."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40 * 96 * 4)
    x = torch.arange(100 * 96, dtype=torch.float32).reshape(100, 1, 32, 3)
    bench.dump_outputs(str(tmp_path / "a"), {"iterates": x})
    bench.dump_outputs(str(tmp_path / "b"), {"iterates": x})
    a, b = np.load(tmp_path / "a" / "iterates.npy"), np.load(tmp_path / "b" / "iterates.npy")
    assert a.shape == (40, 1, 32, 3) and a.nbytes <= bench.DUMP_MAX_BYTES
    np.testing.assert_array_equal(a, b)
    rows = a[:, 0, 0, 0] / 96
    assert np.all(np.diff(rows) > 0) and np.all(rows == np.round(rows))      # whole rows of x, in order
    np.testing.assert_array_equal(a, x.numpy()[rows.astype(int)])
