"""Scalar-quantised index (uint8 codes, exact integer k-NN): one JSON line.

    python tools/sq8_bench.py [--rows 1000000] [--dim 768] [--k 10] [--reps 20]

Rows are drawn on the device (uniform in [-0.5, 0.5)) in pieces, the bounds trained on the first piece, so a large corpus needs
no host array.  Reported: encode GB/s (f32 bytes read per second by lb_gpu_sq8_encode_device); the p50 of a single-query and
of a 1024-query search through the device-pointer entry point, timed by HIP events around the call's own stream work (the
call returns when the results are on the device); for the single query the bytes per second over n * stride + 4 n (what the
distance pass reads and writes) and over that plus 5 * 4 n (the selection's reads of S); for 1024 queries the dot4 operations
per second (n * nq * stride / 4 per pass).  The shader clock is read before and after (measuring-on-mi355x: a number without
its clock is not comparable).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import gpu, sq8  # noqa: E402


def timed(fn, reps):
    """p50 ms by HIP events on the current torch stream; fn synchronises its own stream before it returns"""
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    torch.manual_seed(0)
    enc = sq8.SQ8Encoder(a.dim)
    stride = (a.dim + 15) // 16 * 16
    enc.reserve(a.rows)
    out = {"rows": a.rows, "dim": a.dim, "k": a.k, "stride": stride, "code_bytes": a.rows * stride,
           "shader_clock_mhz_before": clock_mhz()}
    piece = min(a.rows, 1_000_000)
    for r0 in range(0, a.rows, piece):
        cnt = min(piece, a.rows - r0)
        V = torch.rand((cnt, a.dim), device="cuda") - 0.5
        torch.cuda.synchronize()
        if r0 == 0:
            enc.train_device(cnt, V.data_ptr())
            C = torch.empty((cnt, a.dim), dtype=torch.uint8, device="cuda")
            ms = timed(lambda: enc.encode_device(cnt, V.data_ptr(), C.data_ptr()), a.reps)
            out["encode_ms"] = ms
            out["encode_gb_per_s"] = cnt * a.dim * 4 / ms / 1e6
            del C
        enc.add_vectors_device(cnt, V.data_ptr())
        del V
    Q = torch.rand((1024, a.dim), device="cuda") - 0.5
    D = torch.empty((1024, a.k), dtype=torch.float32, device="cuda")
    L = torch.empty((1024, a.k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    res = {}
    for nq in (1, 1024):
        reps = max(3, a.reps // (4 if nq >= 256 else 1))
        ms = timed(lambda: enc.search_device(nq, Q.data_ptr(), a.k, D.data_ptr(), L.data_ptr()), reps)
        r = {"p50_ms": ms}
        if nq == 1:
            r["distance_pass_bytes"] = a.rows * stride + 4 * a.rows
            r["search_bytes"] = a.rows * stride + 4 * a.rows + 5 * 4 * a.rows
            r["distance_pass_bytes_over_search_time_gb_per_s"] = r["distance_pass_bytes"] / ms / 1e6
            r["search_bytes_gb_per_s"] = r["search_bytes"] / ms / 1e6
        else:
            r["dot4_gops_per_s"] = a.rows * nq * (stride // 4) / ms / 1e6
        res[f"nq_{nq}"] = r
    out["search"] = res
    out["shader_clock_mhz_after"] = clock_mhz()
    print(json.dumps(out))
    enc.Close()


if __name__ == "__main__":
    main()
