#!/usr/bin/env python3
"""Coarse-quantiser training on one MI355X: lb_gpu_ivf_train_device over resident rows -- the whole call, the iterations it ran,
the wall time per iteration, and the first iteration's E-step / ordering / M-step (HIP events, lb_gpu_ivf_train_last_timing).
With --nlist <= 256 the same process also runs lb_gpu_pq_train_device with M = 1 on the same rows and init rows, the two calls
alternating, compares the bytes and reports lb_gpu_pq_train_last_timing beside it: the yardstick of the new E-step.

The E-step's floor is 3 * n * nlist * dims lane-operations (a subtract, a multiply and an add per element of every pair, none
fused) over the f32 vector rate without FMA.  The 157.3 TFLOP/s vector peak counts packed FMAs: 256 CUs x 64 lanes x 2 (packed)
x 2 (fused) x 2.4 GHz.  The kernel's arithmetic compiles to v_pk_add_f32 / v_pk_mul_f32 throughout, so its floor is over the
packed rate, 78.6e12 lane-operations/s (half the peak); the floor over the plain rate, 39.3e12 (a quarter), is reported beside
it as "estep_plain_floor_ms".

Every shape is measured in a child process of its own under a time limit (--timeout seconds); a child that fails or runs out of
time ends the run, and nothing more is started.  Prints one JSON line per shape.

usage: python tools/ivf_train_bench.py [--shape N,DIMS,NLIST ...] [--iters 1] [--reps 5] [--timeout 300] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_PLAIN_LANE_OPS_PER_S = 256 * 64 * 2.4e9
F32_LANE_OPS_PER_S = 2 * F32_PLAIN_LANE_OPS_PER_S  # packed, not fused


def med(v):
    return sorted(v)[len(v) // 2]


def worker(n, dims, nlist, max_iter, reps):
    import numpy as np
    import torch

    from longbow_amd import _lib, ivf, pq

    lib = _lib.require_gpu(0)
    X = torch.empty((n, dims), device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), X.numel(), 12345, 0, None))  # splitmix64 rows
    torch.cuda.synchronize()
    rows = np.random.default_rng(7).permutation(n)[:nlist].astype(np.int64)
    parent = nlist <= ivf.TRAIN_MAX_NLIST
    new = {"call": [], "e": [], "o": [], "m": []}
    old = {"call": [], "e": [], "o": [], "m": []}
    ms = (C.c_float * 3)()
    equal, iters = True, 0
    for rep in range(reps + 1):  # the first round also loads the code objects: not counted
        t0 = time.perf_counter()
        cent, iters = ivf.train_coarse_device(n, X.data_ptr(), dims, nlist, max_iter, 1, rows, return_iters=True)
        dt = (time.perf_counter() - t0) * 1e3  # (the call returns after its stream has drained)
        lib.lb_gpu_ivf_train_last_timing(ms)
        if rep:
            new["call"].append(dt); new["e"].append(ms[0]); new["o"].append(ms[1]); new["m"].append(ms[2])
        if parent:
            t0 = time.perf_counter()
            blob, piters = pq.train_device(n, X.data_ptr(), dims, 1, nlist, max_iter, 1, rows.reshape(1, nlist))
            dt = (time.perf_counter() - t0) * 1e3
            lib.lb_gpu_pq_train_last_timing(ms)
            if rep:
                old["call"].append(dt); old["e"].append(ms[0]); old["o"].append(ms[1]); old["m"].append(ms[2])
            equal = equal and blob[12:] == cent.tobytes() and int(piters[0]) == iters
    floor_ms = 3.0 * n * nlist * dims / F32_LANE_OPS_PER_S * 1e3
    out = {"n": n, "dims": dims, "nlist": nlist, "max_iter": max_iter, "reps": reps, "iters_run": iters,
           "call_ms": round(med(new["call"]), 3), "wall_per_iteration_ms": round(med(new["call"]) / max(iters, 1), 3),
           "estep_ms": round(med(new["e"]), 3), "ordering_ms": round(med(new["o"]), 3), "mstep_ms": round(med(new["m"]), 3),
           "estep_floor_ms": round(floor_ms, 3), "estep_share_of_floor": round(floor_ms / med(new["e"]), 4),
           "f32_lane_ops_per_s": F32_LANE_OPS_PER_S, "estep_plain_floor_ms": round(2 * floor_ms, 3)}
    if parent:
        out.update({"pq_train_call_ms": round(med(old["call"]), 3), "pq_train_estep_ms": round(med(old["e"]), 3),
                    "pq_train_ordering_ms": round(med(old["o"]), 3), "pq_train_mstep_ms": round(med(old["m"]), 3),
                    "estep_over_pq_train_estep": round(med(new["e"]) / med(old["e"]), 4), "bytes_equal": equal})
    print(json.dumps(out), flush=True)
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="N,DIMS,NLIST (repeatable); default 100000,768,256")
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in (a.shape or ["100000,768,256"])]
    if a.worker:
        return worker(*shapes[0], a.iters, a.reps)
    for n, dims, nlist in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--shape", f"{n},{dims},{nlist}", "--iters", str(a.iters),
               "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"shape {n},{dims},{nlist}: no result within {a.timeout} s; nothing more is started", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if a.out and r.stdout:
            with open(a.out, "a") as f:
                f.write(r.stdout)
        if r.returncode != 0:
            print(f"shape {n},{dims},{nlist}: exit status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
