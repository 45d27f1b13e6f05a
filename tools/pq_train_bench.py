#!/usr/bin/env python3
"""PQ training on one MI355X: the whole lb_gpu_pq_train_device call, one iteration's E-step / ordering / M-step (HIP events,
lb_gpu_pq_train_last_timing) and, in the same run, one lb_gpu_pq_encode_device pass over the same rows.  The encode pass is the
yardstick: the same n*M*K*sub arithmetic plus square roots, no ordering and no M-step.  Prints one JSON line.

usage: python tools/pq_train_bench.py [--n 100000] [--dims 768] [--M 96] [--K 256] [--iters 20] [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from longbow_amd import _lib, pq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100_000)
ap.add_argument("--dims", type=int, default=768)
ap.add_argument("--M", type=int, default=96)
ap.add_argument("--K", type=int, default=256)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

lib = _lib.require_gpu(0)
X = torch.empty((a.n, a.dims), device="cuda")
_lib.check(lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), X.numel(), 12345, 0, None))  # splitmix64 rows
torch.cuda.synchronize()


def med(v):
    return sorted(v)[len(v) // 2]


whole, est, order, mst, iters = [], [], [], [], None
for rep in range(a.reps + 1):  # the first call also loads the code objects: not counted
    t0 = time.perf_counter()
    blob, iters = pq.train_device(a.n, X.data_ptr(), a.dims, a.M, a.K, a.iters, seed=1)
    dt = time.perf_counter() - t0
    ms = (C.c_float * 3)()
    lib.lb_gpu_pq_train_last_timing(ms)
    if rep:
        whole.append(dt * 1e3)
        est.append(ms[0]); order.append(ms[1]); mst.append(ms[2])
out = {"n": a.n, "dims": a.dims, "M": a.M, "K": a.K, "max_iter": a.iters, "iters_run_max": int(iters.max()),
       "train_call_ms": round(med(whole), 3), "estep_ms": round(med(est), 3), "ordering_ms": round(med(order), 3),
       "mstep_ms": round(med(mst), 3)}
out["iteration_ms"] = round(out["estep_ms"] + out["ordering_ms"] + out["mstep_ms"], 3)
if a.K == 256:
    enc = pq.PQEncoder(blob)
    codes = torch.empty((a.n, a.M), dtype=torch.uint8, device="cuda")
    ts = []
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.encode_device(a.n, X.data_ptr(), codes.data_ptr())  # (returns after the pass: it synchronises its stream)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["encode_pass_ms"] = round(med(ts[1:]), 3)
    out["iteration_over_encode"] = round(out["iteration_ms"] / out["encode_pass_ms"], 3)
    out["estep_over_encode"] = round(out["estep_ms"] / out["encode_pass_ms"], 3)
    enc.Close()
print(json.dumps(out), flush=True)
