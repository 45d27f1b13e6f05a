"""Filtered searches on the BQ, SQ8, PQ, IVF-Flat and IVF-PQ indexes: search time against the share of visible rows, one JSON line.

    python tools/code_filter_bench.py --index bq|sq8|pq|ivf|ivfpq [--rows 1000000] [--dim 768] [--k 100] [--nq 1,64,1024]
                                      [--visible-pct 100,50,10] [--runs 3] [--reps 10] [--nlist 256] [--nprobe 8,32] [--m 96]

BQ and SQ8: rows are drawn on the device (uniform in [-0.5, 0.5)) and added as vectors.  PQ (defaults --rows 10000000,
--nq 1,2,16, --visible-pct 100,50,10,1; M = dim / 8): code bytes uniform in [0, 256) are drawn on the device and added with
add_codes_device, the codebooks are uniform in [0, 1) from seed 7 and so are the queries.  100 % means no filter (the unmapped kernels);
every other share sets a random byte mask with that share of non-zero bytes, so the search walks the list of visible rows.
Per (share, nq): `runs` runs, each the p50 of `reps` searches through the device-pointer entry point (the call returns when the
results are on the device); the figure is the median of the runs, and the runs themselves are kept (their spread is the margin
a comparison between two builds has to clear).  The runs of the shares alternate.  With --visible-pct 100 alone no filter call is
made, so a copy of this file under tools/ of an older checkout times that checkout's unfiltered searches the same way.
The shader clock is read before and after.

IVF-Flat (defaults --nq 1,8, --nprobe 8,32, --visible-pct 100,50,10,1; rows, queries and centroids as tools/ivf_bench.py): here
100 % is a filter too, the all-visible one, because the comparison is another: per (share, nq, nprobe) the search under the
filter, and beside it, in the same run, the same handle with the filter cleared, which is the search of a handle that never had
one.  Each is the p50 of `reps` searches with the HIP-event times of its steps from one more, profiled, search (probes, plan,
list scan, selection) and the rows it scanned.  Per share also the filter call: its wall time (the mask comes from host
memory), the build of the visible lists alone by HIP events, and the bytes that build moves (per list position: the row read
twice, a mask byte gathered, a bit written and read; per visible row 4 bytes written).

IVF-PQ (defaults --rows 10000000, --nlist 1024, --m 96, otherwise as IVF-Flat; rows in pieces of 1M, codebooks and centroids as
tools/ivfpq_bench.py, its queries too): the same comparison and the same figures, with five steps to a search (probes, plan, ADC
tables, scan, selection).  The build reads each row number once (the place step writes positions and loads none).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import _lib, bq, gpu, ivf, ivfpq, pq, sq8  # noqa: E402

DEFAULTS = {"bq": (1_000_000, "1,64,1024", "100,50,10"), "sq8": (1_000_000, "1,64,1024", "100,50,10"),
            "pq": (10_000_000, "1,2,16", "100,50,10,1"), "ivf": (1_000_000, "1,8", "100,50,10,1"),
            "ivfpq": (10_000_000, "1,8", "100,50,10,1")}  # rows, nq, visible-pct
NLIST = {"ivf": 256, "ivfpq": 1024}


def p50(fn, reps):
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


def ivf_handle(a, lib, nqmax):
    """-> (IVFFlat with a.rows rows, queries [nqmax, dim] on the device): rows, queries and centroids as tools/ivf_bench.py"""
    X = torch.empty((a.rows, a.dim), dtype=torch.float32, device="cuda")
    Q = torch.empty((nqmax, a.dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), a.rows * a.dim, 1, 0, None))
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), nqmax * a.dim, 2, 0, None))
    torch.cuda.synchronize()
    h = ivf.IVFFlat(ivf.train_device(a.rows, X.data_ptr(), a.dim, a.nlist, max_iter=0))
    h.reserve(a.rows)
    h.add_device(a.rows, X.data_ptr())
    return h, Q


def ivfpq_handle(a, lib, nqmax):
    """-> (IVFPQ with a.rows rows, queries [nqmax, dim] on the device): rows, codebooks, centroids and queries as
    tools/ivfpq_bench.py"""
    n, dim, M, piece = a.rows, a.dim, a.m, 1_000_000
    cb = torch.empty(M * 256 * (dim // M), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, cb.data_ptr(), cb.numel(), 7, 0, None))
    rows = torch.arange(a.nlist, dtype=torch.int64, device="cuda") * (n // a.nlist)
    cent = torch.empty((a.nlist, dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_rows_device(0, cent.data_ptr(), rows.data_ptr(), a.nlist, dim, 12345, None))
    torch.cuda.synchronize()
    h = ivfpq.IVFPQ(pq.serialize_codebooks(cb.cpu().numpy().reshape(M, 256, dim // M)), cent.cpu().numpy())
    h.reserve(n)
    buf = torch.empty((min(piece, n), dim), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, piece):
        cnt = min(piece, n - r0)
        _lib.check(lib.lb_gpu_fill_uniform_device(0, buf.data_ptr(), cnt * dim, 12345, r0 * dim, None))
        torch.cuda.synchronize()
        h.add_device(cnt, buf.data_ptr())
    Q = torch.empty((nqmax, dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), nqmax * dim, 42, 0, None))
    torch.cuda.synchronize()
    return h, Q


def ivf_main(a, nqs, pcts):
    lib = _lib.require_gpu(0)
    nprobes = [int(x) for x in a.nprobe.split(",")]
    out = {"index": a.index, "rows": a.rows, "dim": a.dim, "nlist": a.nlist, "k": a.k, "runs": a.runs, "reps": a.reps,
           "shader_clock_mhz_before": clock_mhz()}
    nqmax = max(nqs)
    if a.index == "ivfpq":
        out["m"] = a.m
        h, Q = ivfpq_handle(a, lib, nqmax)
    else:
        h, Q = ivf_handle(a, lib, nqmax)
    slots = h._timing_slots
    rng = np.random.default_rng(0)
    masks = {p: np.ones(a.rows, np.uint8) if p == 100 else (rng.random(a.rows) < p / 100.0).astype(np.uint8) for p in pcts}
    D = torch.empty((nqmax, a.k), dtype=torch.float32, device="cuda")
    L = torch.empty((nqmax, a.k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def cell(nq, nprobe):
        run = lambda: h.search_device(nq, Q.data_ptr(), a.k, nprobe, D.data_ptr(), L.data_ptr())  # noqa: E731
        ms = p50(run, a.reps)
        h.set_profiling(True)
        run()
        h.set_profiling(False)
        st = h.last_search_stats()
        return {"ms": ms, "steps_ms": list(h.last_timing()), "rows_scanned": st[1], "max_rows_per_query": st[2], "selected_from_lds": st[3]}

    grid = [(nq, nprobe) for nq in nqs for nprobe in nprobes]
    runs = {p: {"filter_call_ms": [], "build_ms": [], "cells": {g: {"filtered": [], "unfiltered": []} for g in grid}} for p in pcts}
    for _ in range(a.runs):
        for p in pcts:
            r = runs[p]
            h.set_filter(None)
            for g in grid:
                r["cells"][g]["unfiltered"].append(cell(*g))
            h.set_filter(masks[p])  # (warm: the buffers exist from here on)
            h.set_filter(None)
            t0 = time.perf_counter()
            h.set_filter(masks[p])
            r["filter_call_ms"].append((time.perf_counter() - t0) * 1e3)
            h.set_profiling(True)
            h.set_filter(masks[p])
            h.set_profiling(False)
            r["build_ms"].append(h.last_build_timing())
            r["visible_rows"] = h.nvisible()
            for g in grid:
                r["cells"][g]["filtered"].append(cell(*g))
    med = lambda xs: float(np.median(xs))  # noqa: E731

    def summary(cs):
        return {"ms": med([c["ms"] for c in cs]), "runs_ms": [c["ms"] for c in cs],
                "steps_ms": [med([c["steps_ms"][i] for c in cs]) for i in range(slots)],
                "rows_scanned": cs[-1]["rows_scanned"], "max_rows_per_query": cs[-1]["max_rows_per_query"],
                "selected_from_lds": cs[-1]["selected_from_lds"]}

    out["filter"] = {}
    for p in pcts:
        r = runs[p]
        build_bytes = a.rows * (4 + 1 + (0 if a.index == "ivfpq" else 4)) + a.rows // 4 + r["visible_rows"] * 4
        out["filter"][f"visible_{p}"] = {
            "visible_rows": r["visible_rows"], "filter_call_ms": med(r["filter_call_ms"]), "filter_call_runs_ms": r["filter_call_ms"],
            "build_ms": med(r["build_ms"]), "build_runs_ms": r["build_ms"], "build_bytes": build_bytes,
            "build_gb_per_s": build_bytes / max(med(r["build_ms"]), 1e-6) / 1e6,
            "search": {f"nq_{nq}_nprobe_{nprobe}": {k: summary(v) for k, v in r["cells"][(nq, nprobe)].items()} for nq, nprobe in grid}}
    out["hbm_bytes"] = h.hbm_bytes
    out["shader_clock_mhz_after"] = clock_mhz()
    print(json.dumps(out))
    h.Close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", choices=("bq", "sq8", "pq", "ivf", "ivfpq"), required=True)
    ap.add_argument("--nlist", type=int, default=None)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--nprobe", default="8,32")
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nq", default=None)
    ap.add_argument("--visible-pct", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    a.rows = a.rows if a.rows is not None else DEFAULTS[a.index][0]
    a.nq = a.nq or DEFAULTS[a.index][1]
    a.visible_pct = a.visible_pct or DEFAULTS[a.index][2]
    nqs = [int(x) for x in a.nq.split(",")]
    pcts = [int(x) for x in a.visible_pct.split(",")]
    if a.index in NLIST:
        a.nlist = a.nlist or NLIST[a.index]
        return ivf_main(a, nqs, pcts)
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    if a.index == "pq":
        M = a.dim // 8
        enc = pq.PQEncoder(pq.serialize_codebooks(np.random.default_rng(7).random((M, 256, 8), dtype=np.float32)))
    else:
        enc = bq.BQEncoder(a.dim) if a.index == "bq" else sq8.SQ8Encoder(a.dim)
    enc.reserve(a.rows)
    out = {"index": a.index, "rows": a.rows, "dim": a.dim, "k": a.k, "runs": a.runs, "reps": a.reps,
           "shader_clock_mhz_before": clock_mhz()}
    piece = min(a.rows, 1_000_000)
    for r0 in range(0, a.rows, piece):
        cnt = min(piece, a.rows - r0)
        if a.index == "pq":
            V = torch.randint(0, 256, (cnt, enc.M), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            enc.add_codes_device(cnt, V.data_ptr())
            del V
            continue
        V = torch.rand((cnt, a.dim), device="cuda") - 0.5
        torch.cuda.synchronize()
        if r0 == 0 and a.index == "sq8":
            enc.train_device(cnt, V.data_ptr())
        enc.add_vectors_device(cnt, V.data_ptr())
        del V
    masks = {p: (rng.random(a.rows) < p / 100.0).astype(np.uint8) for p in pcts if p != 100}
    nqmax = max(nqs)
    Q = torch.rand((nqmax, a.dim), device="cuda") - (0.0 if a.index == "pq" else 0.5)
    D = torch.empty((nqmax, a.k), dtype=torch.float32, device="cuda")
    L = torch.empty((nqmax, a.k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    runs = {p: {nq: [] for nq in nqs} for p in pcts}
    visible = {}
    for _ in range(a.runs):
        for p in pcts:
            if p == 100:
                if masks:
                    enc.set_filter(None)
                visible[p] = a.rows
            else:
                enc.set_filter(masks[p])
                visible[p] = enc.nvisible()
            for nq in nqs:
                runs[p][nq].append(p50(lambda: enc.search_device(nq, Q.data_ptr(), a.k, D.data_ptr(), L.data_ptr()), a.reps))
    out["search"] = {f"visible_{p}": {"visible_rows": visible[p],
                                      **{f"nq_{nq}": {"ms": float(np.median(runs[p][nq])), "runs_ms": runs[p][nq]} for nq in nqs}}
                     for p in pcts}
    out["shader_clock_mhz_after"] = clock_mhz()
    print(json.dumps(out))
    enc.Close()


if __name__ == "__main__":
    main()
