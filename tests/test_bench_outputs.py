"""bench.py --dump-outputs DIR: what the timed path returned in its last step, as DIR/<name>.npy (float32 / float64, at most
64 MB in all), --steps as the number of timed steps behind ms_per_step, and what a plain run's line holds beside one with --full."""
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
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "20000", "--batch", "64", "--full", "--no-legs", "--no-fast",
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


# what a run without --full prints: the headline, its configuration, and what the timed steps' own HIP events give
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "full",
              "vs_baseline", "dtype", "data", "config", "fallback_queries", "device_ms_per_step", "roofline"}


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_and_runs_no_other_leg(tmp_path):
    from tests.gpu_util import gpu_or_skip
    gpu_or_skip()
    out = tmp_path / "dump"
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "20000", "--batch", "64", "--dump-outputs", str(out)],
             timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert set(res) <= PLAIN_KEYS, sorted(set(res) - PLAIN_KEYS)  # no parity, latency, sweep, CPU baseline, strong C3, configs 1 / 4 / 5
    assert res["full"] is False and res["steps"] == 3 and res["warmup"] == 1
    assert res["metric"].startswith("k-NN queries/sec") and res["unit"] == "queries/s" and res["dtype"] == "f32"
    assert res["higher_is_better"] is True and res["ms_per_step"] > 0
    # value is in queries over 1M rows; ms_per_step is printed to 1e-4 ms and a step of several launches takes over 0.02 ms
    assert res["value"] == pytest.approx(64 * (20000 / 1e6) * 1e3 / res["ms_per_step"], rel=5e-3)
    lab, dist = np.load(out / "labels.npy"), np.load(out / "distances.npy")  # the dump does not wait for --full
    assert lab.dtype == np.float64 and dist.dtype == np.float32 and lab.shape == dist.shape == (64, 100)
    assert np.all((lab >= 0) & (lab < 20000) & (lab == np.round(lab))) and np.all(np.diff(dist, axis=1) >= 0)
