"""float16 index vs float32 index over the same (widened) data: one JSON line.

    python tools/f16_index_bench.py [--rows 1000000] [--dim 768] [--reps 20]

Per metric: p50 of single-query searches and ms per batch at 1 / 64 / 1024 queries (k = 10), last_route and hbm_bytes, for an
F16 index and for an f32 index over the widened rows.  Both take the fp16-image routes for batches (63 / 73); the F16 index's
image is a relayout of its rows.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    X16 = rng.standard_normal((a.rows, a.dim), dtype=np.float32).astype(np.float16)
    Q16 = rng.standard_normal((1024, a.dim), dtype=np.float32).astype(np.float16)
    X32, Q32 = X16.astype(np.float32), Q16.astype(np.float32)
    out = {"rows": a.rows, "dim": a.dim, "k": 10, "metrics": {}}
    for metric, name in ((0, "l2"), (1, "cosine"), (2, "dot")):
        res = {}
        for dt, X, Q in ((gpu.DataType.Float16, X16, Q16), (gpu.DataType.Float32, X32, Q32)):
            idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=a.dim, Metric=metric, DataType=dt))
            idx.Add(None, X)
            r = {"p50_single_ms": timed(lambda: idx.Search(Q[0], 10), a.reps)}
            routes = {}
            for b in (1, 64, 1024):
                r[f"ms_batch_{b}"] = timed(lambda: idx.SearchBatch(Q[:b], 10), max(3, a.reps // (4 if b == 1024 else 1)))
                routes[str(b)] = int(idx._lib.lb_gpu_index_last_route(idx._h))
            r["last_route"] = routes
            r["hbm_bytes"] = idx.hbm_bytes()
            res["f16" if dt == gpu.DataType.Float16 else "f32"] = r
            idx.Close()
        out["metrics"][name] = res
    try:
        out["shader_clock_mhz"] = float(gpu._lib.load().lb_gpu_shader_clock_mhz(0, 2000))
    except Exception:
        pass
    print(json.dumps(out))


if __name__ == "__main__":
    main()
