"""bench.py --dump-outputs DIR: what the timed path returned in its last step, as DIR/<name>.npy (float32 / float64, at most
64 MB in all), and --steps as the number of timed steps behind ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _run(args, timeout):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LB_BENCH_CHILD", "LB_BENCH_LAUNCH_ECHO"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout, cwd=ROOT)


def test_dump_writes_float_arrays_exactly(tmp_path):
    bench = _bench()
    lab = np.array([[3, 1, -1], [2 ** 40, 0, 7]], np.int64)
    dist = np.array([[0.5, 1.25, np.finfo(np.float32).max], [0.0, 2.0, 3.0]], np.float32)
    bench.dump_outputs(str(tmp_path / "out"), {"labels": lab, "distances": dist})
    assert sorted(os.listdir(tmp_path / "out")) == ["distances.npy", "labels.npy"]
    got_l, got_d = np.load(tmp_path / "out" / "labels.npy"), np.load(tmp_path / "out" / "distances.npy")
    assert got_l.dtype == np.float64 and np.array_equal(got_l.astype(np.int64), lab)
    assert got_d.dtype == np.float32 and np.array_equal(got_d, dist)


def test_dump_over_the_cap_is_a_fixed_row_sample(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 20_000)
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 1 << 20, (1000, 10)).astype(np.int64)
    dist = rng.random((1000, 10), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"labels": lab, "distances": dist})
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in os.listdir(tmp_path / "a")) <= 20_000
    rows = np.load(tmp_path / "a" / "query_rows.npy")
    assert rows.dtype == np.float64 and 0 < rows.size < 1000 and np.all(np.diff(rows) > 0)
    sel = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "labels.npy"), lab[sel].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "distances.npy"), dist[sel])
    for f in ("query_rows.npy", "labels.npy", "distances.npy"):  # the same sample on every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_steps_below_one_are_refused_before_the_gpu():
    r = _run(["--gpus", "1", "--steps", "0"], timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    from tests.gpu_util import gpu_or_skip
    gpu_or_skip()
    out = tmp_path / "dump"
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "20000", "--batch", "64", "--no-legs", "--no-fast",
              "--no-cpu-baseline", "--dump-outputs", str(out)], timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    assert res["parity"]["ok"], res["parity"]  # the dumped lists are the ones the oracle checked
    lab, dist = np.load(out / "labels.npy"), np.load(out / "distances.npy")
    assert lab.dtype == np.float64 and dist.dtype == np.float32
    assert lab.shape == dist.shape == (64, 100)
    assert np.all((lab >= 0) & (lab < 20000) & (lab == np.round(lab)))
    assert np.all(np.diff(dist, axis=1) >= 0)
