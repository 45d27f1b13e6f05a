"""uint8 index vs the int8 index over the same bytes shifted by 128 and the float32 index over the widened values: one JSON line.

    python tools/u8_index_bench.py [--rows 1000000] [--dim 768] [--reps 20] [--k 10] [--corpora uniform_0_255,narrow_96_160]

Two corpora: uniform bytes 0..255 (at 768 dimensions a share of the pairs has S > 2^24 and takes the drop test or the chain
recompute) and bytes drawn from 96..160 (no pair leaves the integer path).  Per corpus, first the three indexes' labels are
asserted equal for 64 queries (the uint8 and float32 distances too: below 2^24 both are sqrt of the same exact integer; the
int8 index's kernel rounds its integer sum once, which is the same value there; beyond 2^24, as for uniform bytes at 1536
dimensions where E[S] is about 2^24, only the labels are asserted), then per batch of 1 / 16 / 64 / 256 / 1024 queries the p50
and the [min, max] ms of a search and the route it took (82 scan, 83 matrix-core pass for the uint8 index), and hbm_bytes.  For
the uint8 index's batches of 64 and 1024 one profiled search also gives the share of the device time spent outside the main
corpus pass (sample pass, thresholds and select).  The uint8 and int8 indexes read the same HBM bytes, so their times are the
comparison of interest.  In the diagnostic build (LB_GPU_SO=.../liblongbow_gpu_diag.so) LB_U8_MFMA_MINQ above the batch keeps
the uint8 index on the scan.  The shader clock is read before and after the timings.
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--corpora", default="uniform_0_255,narrow_96_160")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    out = {"rows": a.rows, "dim": a.dim, "k": a.k, "shader_clock_mhz_before": clock_mhz(), "corpora": {}}
    for name, lo, hi in (("uniform_0_255", 0, 256), ("narrow_96_160", 96, 161)):
        if name not in a.corpora.split(","):
            continue
        X = rng.integers(lo, hi, (a.rows, a.dim), dtype=np.int64).astype(np.uint8)
        Q = rng.integers(lo, hi, (1024, a.dim), dtype=np.int64).astype(np.uint8)
        forms = (("u8", gpu.DataType.Uint8, lambda v: v), ("i8", gpu.DataType.Int8, lambda v: (v ^ 0x80).view(np.int8)),
                 ("f32", gpu.DataType.Float32, lambda v: v.astype(np.float32)))
        res, first = {}, None
        for tag, dt, conv in forms:
            cfg = gpu.GPUConfig(DeviceID=0, Dimension=a.dim, Metric=0, DataType=dt)
            idx = gpu.NewUint8Index(cfg) if tag == "u8" else gpu.NewIndexWithConfig(cfg)
            Xc, Qc = conv(X), conv(Q)
            idx.Add(None, Xc)
            del Xc
            lab, dist = idx.SearchBatch(Qc[:64], a.k)
            if first is None:
                first = (lab, dist)
            else:  # equal results before any timing
                assert np.array_equal(lab, first[0]), f"{name}: {tag} labels differ from the uint8 index's"
                res.setdefault("distances_equal_u8", {})[tag] = bool(np.array_equal(dist, first[1]))
            r, routes = {}, {}
            for b in (1, 16, 64, 256, 1024):
                r[f"ms_batch_{b}"], lo_ms, hi_ms = timed(lambda: idx.SearchBatch(Qc[:b], a.k), max(3, a.reps // (4 if b >= 256 else 1)))
                r[f"ms_batch_{b}_min_max"] = [lo_ms, hi_ms]
                routes[str(b)] = int(idx._lib.lb_gpu_index_last_route(idx._h))
                if tag == "u8" and b in (64, 1024):
                    idx.set_profiling(True)
                    idx.SearchBatch(Qc[:b], a.k)
                    t = idx.last_timing()
                    idx.set_profiling(False)
                    r[f"share_outside_main_pass_{b}"] = t["select"][0] / max(t["select"][0] + t["scan"][0] + t["gemm"][0] + t["rerank"][0], 1e-9)
            r["last_route"] = routes
            r["hbm_bytes"] = idx.hbm_bytes()
            res[tag] = r
            idx.Close()
        out["corpora"][name] = res
    out["shader_clock_mhz_after"] = clock_mhz()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
