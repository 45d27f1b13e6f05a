"""int8 index vs float32 index over the same (widened) data: one JSON line.

    python tools/i8_index_bench.py [--rows 1000000] [--dim 768] [--reps 20]

Per metric (L2, dot) and k in {10, 100}: p50 ms per search of 1 / 64 / 1024 queries, last_route and hbm_bytes, for an int8
index (routes 80: exact scan, 81: i8 MFMA pass) and for an f32 index over the widened rows.  The shader clock is read before
and after the timings (measuring-on-mi355x: a number without its clock is not comparable).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import gpu  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def clock_mhz():
    try:
        return float(gpu._lib.load().lb_gpu_shader_clock_mhz(0, 2000))
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    X8 = rng.integers(-128, 128, (a.rows, a.dim), dtype=np.int64).astype(np.int8)
    Q8 = rng.integers(-128, 128, (1024, a.dim), dtype=np.int64).astype(np.int8)
    X32, Q32 = X8.astype(np.float32), Q8.astype(np.float32)
    out = {"rows": a.rows, "dim": a.dim, "shader_clock_mhz_before": clock_mhz(), "metrics": {}}
    for metric, name in ((0, "l2"), (2, "dot")):
        res = {}
        for dt, X, Q in ((gpu.DataType.Int8, X8, Q8), (gpu.DataType.Float32, X32, Q32)):
            idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=a.dim, Metric=metric, DataType=dt))
            idx.Add(None, X)
            r, routes = {}, {}
            for k in (10, 100):
                for b in (1, 64, 1024):
                    r[f"k{k}_ms_batch_{b}"] = timed(lambda: idx.SearchBatch(Q[:b], k), max(3, a.reps // (4 if b == 1024 else 1)))
                    routes[f"k{k}_{b}"] = int(idx._lib.lb_gpu_index_last_route(idx._h))
            r["last_route"] = routes
            r["hbm_bytes"] = idx.hbm_bytes()
            res["i8" if dt == gpu.DataType.Int8 else "f32"] = r
            idx.Close()
        out["metrics"][name] = res
    out["shader_clock_mhz_after"] = clock_mhz()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
