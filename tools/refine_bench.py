"""Batched exact refine of shortlists (lb_gpu_index_refine) on a float32 and a float16 index of the same rows: one JSON line.

    python tools/refine_bench.py [--rows 1000000] [--dim 768] [--k 100] [--nq 1 8 64 1024] [--c 100 1000]

Rows and queries come from the seeded device fill (uniform in [-0.5, 0.5)); the float16 index holds the same rows rounded to
fp16.  A shortlist is c random rows (with the few repeats that gives).  Per cell (element type x nq x c): the median of three
runs, each the p50 of ten calls after a warm-up, of the device-pointer entry point by wall clock (the call returns when the
results are on the device) and of the host-pointer one; the HIP-event time of each launch from one more, profiled, call
(prepare, scan, selection); the bytes the scan gathers (the distinct rows of every shortlist x D x the element size) over the
scan's time, and that rate as a fraction of --yardstick-tbs (5.5: the low end of what a random whole-row gather into registers
reaches on this part).  Beside every float32 cell, in the same run: the per-query path over the same shortlists, one
lb_gpu_index_rerank call and one host sort per query, as sq8.search_rerank does it.  The shader clock is read before and after.
A run that finds no GPU fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import _lib, gpu  # noqa: E402


def p50_ms(fn, reps=10):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def median_of_p50s(fn, runs=3, reps=10):
    fn()
    fn()
    return float(np.median([p50_ms(fn, reps) for _ in range(runs)]))


def clock_mhz(lib):
    try:
        return float(lib.lb_gpu_shader_clock_mhz(0, 2000))
    except Exception:
        return None


def rerank_loop(idx, Q, rows, k):
    """today's second stage: a call and a host sort per query"""
    for q in range(Q.shape[0]):
        r = rows[q]
        d = idx.Rerank(Q[q], r, order=None, want_score=False)
        np.lexsort((r, d))[:k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--piece", type=int, default=250_000)
    ap.add_argument("--nq", type=int, nargs="*", default=[1, 8, 64, 1024])
    ap.add_argument("--c", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--yardstick-tbs", type=float, default=5.5)
    a = ap.parse_args()
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, dim, k = a.rows, a.dim, a.k
    out = {"rows": n, "dim": dim, "k": k, "yardstick_tb_per_s": a.yardstick_tbs, "shader_clock_mhz_before": clock_mhz(lib)}
    f32 = gpu.Index(gpu.GPUConfig(DeviceID=0, Dimension=dim))
    f16 = gpu.Index(gpu.GPUConfig(DeviceID=0, Dimension=dim, DataType=gpu.DataType.Float16))
    for idx in (f32, f16):
        idx.reserve(n)
    buf = torch.empty((min(a.piece, n), dim), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, a.piece):
        cnt = min(a.piece, n - r0)
        _lib.check(lib.lb_gpu_fill_uniform_device(0, buf.data_ptr(), cnt * dim, 12345, r0 * dim, None))
        torch.cuda.synchronize()
        f32.add_device(cnt, buf.data_ptr())
        half = buf[:cnt].half().contiguous()
        torch.cuda.synchronize()
        f16.add_device(cnt, half.data_ptr())
        del half
    del buf
    nqmax = max(a.nq)
    Q = torch.empty((nqmax, dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), nqmax * dim, 42, 0, None))
    D = torch.empty((nqmax, k), dtype=torch.float32, device="cuda")
    L = torch.empty((nqmax, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    Qh = Q.cpu().numpy()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    cells = []
    for c in a.c:
        R = torch.randint(0, n, (nqmax, c), generator=gen, device="cuda", dtype=torch.int64)
        torch.cuda.synchronize()
        Rh = R.cpu().numpy()
        distinct = np.array([np.unique(r).size for r in Rh], np.int64)
        for nq in a.nq:
            ref = None
            for name, idx, elem in (("float32", f32, 4), ("float16", f16, 2)):
                dev = lambda: idx.refine_device(nq, Q.data_ptr(), c, R.data_ptr(), k, D.data_ptr(), L.data_ptr())  # noqa: E731
                host = lambda: idx.Refine(Qh[:nq], Rh[:nq], k)  # noqa: E731
                ms = median_of_p50s(dev)
                host_ms = median_of_p50s(host, reps=5 if nq > 64 else 10)
                idx.set_profiling(True)
                dev()
                idx.set_profiling(False)
                steps = idx.refine_last_timing()
                gathered = int(distinct[:nq].sum()) * dim * elem
                rate = gathered / max(steps[1], 1e-6) / 1e9  # TB/s
                cell = {"rows_dtype": name, "nq": nq, "c": c, "p50_ms": ms, "host_pointer_p50_ms": host_ms,
                        "prepare_ms": steps[0], "scan_ms": steps[1], "select_ms": steps[2], "bytes_gathered": gathered,
                        "scan_tb_per_s": rate, "fraction_of_yardstick": rate / a.yardstick_tbs}
                got = (L[:nq].cpu().numpy(), D[:nq].cpu().numpy())
                if name == "float32":
                    ref = got
                    loop = lambda: rerank_loop(f32, Qh[:nq], Rh[:nq], k)  # noqa: E731
                    cell["rerank_loop_p50_ms"] = median_of_p50s(loop, reps=3 if nq > 64 else 10)
                    cell["host_pointer_speedup_over_loop"] = cell["rerank_loop_p50_ms"] / host_ms
                else:
                    cell["labels_shared_with_float32"] = float(np.mean([np.intersect1d(got[0][j], ref[0][j]).size / k for j in range(nq)]))
                cells.append(cell)
    out["cells"] = cells
    out["shader_clock_mhz_after"] = clock_mhz(lib)
    print(json.dumps(out))
    f32.Close()
    f16.Close()


if __name__ == "__main__":
    main()
