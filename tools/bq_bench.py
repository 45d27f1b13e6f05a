"""Binary-quantised index (sign-bit codes, exact Hamming k-NN) beside the float32 index over the same rows: one JSON line.

    python tools/bq_bench.py [--rows 1000000] [--dim 768] [--k 100] [--reps 20] [--no-f32]

Rows are drawn on the device (uniform in [-0.5, 0.5)) in pieces and added to both indexes, so 10M x 768 needs no 30 GB host
array.  Per nq in {1, 8, 64, 256, 1024}: p50 ms per search through the device-pointer entry points (the call returns when the
results are on the device).  For nq <= 8 the code bytes N*W*8 per second of one search; for the batches the pair-words
(N * nq * W) per second.  Encode GB/s is f32 bytes read per second by lb_gpu_bq_encode_device.  The shader clock is read
before and after (measuring-on-mi355x: a number without its clock is not comparable).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import bq, gpu  # noqa: E402


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
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-f32", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    enc = bq.BQEncoder(a.dim)
    idx = None if a.no_f32 else gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=a.dim, Metric=0))
    enc.reserve(a.rows)
    out = {"rows": a.rows, "dim": a.dim, "k": a.k, "words": enc.W, "code_bytes": a.rows * enc.W * 8,
           "shader_clock_mhz_before": clock_mhz()}
    piece = min(a.rows, 1_000_000)
    for r0 in range(0, a.rows, piece):
        cnt = min(piece, a.rows - r0)
        V = torch.rand((cnt, a.dim), device="cuda") - 0.5
        torch.cuda.synchronize()
        if r0 == 0:
            C = torch.empty((cnt, enc.W), dtype=torch.int64, device="cuda")
            ms = timed(lambda: enc.encode_device(cnt, V.data_ptr(), C.data_ptr()), a.reps)
            out["encode_ms"] = ms
            out["encode_gb_per_s"] = cnt * a.dim * 4 / ms / 1e6
            del C
        enc.add_vectors_device(cnt, V.data_ptr())
        if idx is not None:
            idx.add_device(cnt, V.data_ptr())
        del V
    Q = torch.rand((1024, a.dim), device="cuda") - 0.5
    D = torch.empty((1024, a.k), dtype=torch.float32, device="cuda")
    L = torch.empty((1024, a.k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    res = {}
    for nq in (1, 8, 64, 256, 1024):
        reps = max(3, a.reps // (4 if nq >= 256 else 1))
        r = {"bq_p50_ms": timed(lambda: enc.search_device(nq, Q.data_ptr(), a.k, D.data_ptr(), L.data_ptr()), reps)}
        if nq <= 8:
            r["bq_code_gb_per_s"] = a.rows * enc.W * 8 / r["bq_p50_ms"] / 1e6
        else:
            r["bq_pair_gwords_per_s"] = a.rows * nq * enc.W / r["bq_p50_ms"] / 1e6
        if idx is not None:
            r["f32_p50_ms"] = timed(lambda: idx.search_device(nq, Q.data_ptr(), a.k, D.data_ptr(), L.data_ptr()), reps)
        res[f"nq_{nq}"] = r
    out["search"] = res
    out["shader_clock_mhz_after"] = clock_mhz()
    print(json.dumps(out))
    enc.Close()
    if idx is not None:
        idx.Close()


if __name__ == "__main__":
    main()
