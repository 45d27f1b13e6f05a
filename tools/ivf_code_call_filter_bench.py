"""A row bitmap given with the search call on the IVF-PQ handle, plain or residual, and on the IVF-SQ8 handle
(lb_gpu_ivfpq_search_bitmap_device_ctx, lb_gpu_ivfsq8_search_bitmap_device_ctx), beside what a per-request filter costs without it:
one JSON line.  The code handles' counterpart of tools/ivf_call_filter_bench.py, whose three forms, cells and clocking it takes
as they are.

    python tools/ivf_code_call_filter_bench.py --index ivfpq|ivfpq-residual|ivfsq8 [--rows N] [--dim 768] [--m 96] [--nlist L] [--k 10]

The shapes default to the ones the README quotes for each handle: 10M x 768 in 96-byte codes over 1,024 lists for IVF-PQ, 1M x 768
over 256 lists for IVF-SQ8.  Rows and queries are bench.py's seeded device fill (corpus seed 12345, queries 42), the rows in pieces
of --piece rows that are added with add_device and never held together; the centroids are nlist rows of the same fill, the
codebooks the seeded fill of seed 7 (tools/ivfpq_bench.py's), the SQ8 bounds -0.5 / 0.5, the fill's range.  Everything runs in one
process, and a run that finds no GPU fails.  Before anything is timed, the three forms are compared bit for bit (labels, distances,
last_search_stats) in every cell.

  cells   nq in {1, 64, 1024} x nprobe in {1, 8, 32} x visible in {100 %, 10 %, 1 %} (a random mask of that density)
    a     the bitmap search through device pointers, on a handle without a filter
    b     another handle under set_filter with the identical mask, searched through device pointers
    c     b plus the set_filter call in front of it: what a request that brings its own filter costs without the call
  Beside each cell the profiled slots of one call of `a` and one of `b`: ms[1], the plan, which holds the compaction, ms[2] (the
  tables / the queries' codes), ms[3] the scan and ms[4] the selection; and which form of the compaction the host's rule chose
  ("shared": every list once for the call; else once per query and probe).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_call_filter_bench as flat  # noqa: E402  (the forms, the cells and the clocking)
from longbow_amd import _lib, ivfpq, ivfsq8, pq  # noqa: E402

DEFAULTS = {"ivfpq": (10_000_000, 1024), "ivfpq-residual": (10_000_000, 1024), "ivfsq8": (1_000_000, 256)}


class Forms(flat.Forms):
    def slots(self, nq, nprobe):
        out = {}
        for name, h, fn in (("a", self.ha, self.a(nq, nprobe)), ("b", self.hb, self.b(nq, nprobe))):
            h.set_profiling(True)
            fn()
            fn()
            t = h.last_timing()
            h.set_profiling(False)
            out[name] = {"probes_ms": t[0], "plan_ms": t[1], "tables_ms": t[2], "scan_ms": t[3], "select_ms": t[4]}
        return out


def shared_form(sizes, nq, nprobe):
    """the host's rule (lb_ivf_host.h, ivf_search) under one bitmap"""
    s = np.sort(np.asarray(sizes, np.int64))[::-1]
    return bool(nq * max(int(s[:nprobe].sum()), 1) > int(s.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", choices=sorted(DEFAULTS), required=True)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--nlist", type=int, default=0)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--piece", type=int, default=1_000_000)
    a = ap.parse_args()
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, nlist = a.rows or DEFAULTS[a.index][0], a.nlist or DEFAULTS[a.index][1]
    d, k, M = a.dim, a.k, a.m
    out = {"index": a.index, "rows": n, "dim": d, "nlist": nlist, "k": k, "shader_clock_mhz_before": flat.clock_mhz(lib)}
    Q = torch.empty((1024, d), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), Q.numel(), 42, 0, None))
    rows = torch.arange(nlist, dtype=torch.int64, device="cuda") * (n // nlist)  # the centroids: rows 0, n / nlist, ... of the fill
    cent = torch.empty((nlist, d), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_rows_device(0, cent.data_ptr(), rows.data_ptr(), nlist, d, 12345, None))
    torch.cuda.synchronize()
    cent = cent.cpu().numpy()
    if a.index == "ivfsq8":
        new = lambda: ivfsq8.IVFSQ8(np.full(d, -0.5, np.float32), np.full(d, 0.5, np.float32), cent)
    else:
        out["m"] = M
        cb = torch.empty(M * 256 * (d // M), dtype=torch.float32, device="cuda")
        _lib.check(lib.lb_gpu_fill_uniform_device(0, cb.data_ptr(), cb.numel(), 7, 0, None))
        torch.cuda.synchronize()
        blob = pq.serialize_codebooks(cb.cpu().numpy().reshape(M, 256, d // M))
        new = lambda: ivfpq.IVFPQ(blob, cent, residual=a.index == "ivfpq-residual")
    ha, hb = new(), new()
    buf = torch.empty((min(a.piece, n), d), dtype=torch.float32, device="cuda")
    t0 = time.perf_counter()
    for h in (ha, hb):
        h.reserve(n)
    for r0 in range(0, n, a.piece):
        cnt = min(a.piece, n - r0)
        _lib.check(lib.lb_gpu_fill_uniform_device(0, buf.data_ptr(), cnt * d, 12345, r0 * d, None))
        torch.cuda.synchronize()
        for h in (ha, hb):
            h.add_device(cnt, buf.data_ptr())
    out["add_seconds_both_handles"] = time.perf_counter() - t0
    del buf
    sizes = ha.list_sizes()
    out["list_sizes"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max())}
    rng = np.random.default_rng(1)
    score = rng.random(n)  # row r is visible at p % iff score[r] < p / 100: nested masks
    f = Forms(ha, hb, Q, k)
    table = {}
    for pct in flat.VISIBLE:
        f.set_mask((score < pct / 100.0).astype(np.uint8))
        out[f"visible_rows_{pct}pct"] = int(f.mask.sum())
        for nq in flat.NQS:
            for nprobe in flat.NPROBES:
                st = f.verify(nq, nprobe, f"{pct} % visible, {nq} queries, {nprobe} probes")
                cell = f.cell(nq, nprobe)
                cell["rows_scanned"] = st[1]
                cell["shared"] = shared_form(sizes, nq, nprobe)
                table[f"vis{pct}_q{nq}_nprobe{nprobe}"] = cell
                print(f"vis{pct}_q{nq}_nprobe{nprobe}", json.dumps(cell), file=sys.stderr, flush=True)
        assert ha.nvisible() == n  # the handle searched under bitmaps never had a filter
    out["cells"] = table
    t0 = time.perf_counter()
    hb.set_filter(f.mask)
    out["set_filter_ms_last_mask"] = (time.perf_counter() - t0) * 1e3
    ha.Close()
    hb.Close()
    out["shader_clock_mhz_after"] = flat.clock_mhz(lib)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
