"""A row bitmap given with the search call on the IVF-Flat handle (lb_gpu_ivf_search_bitmap_device_ctx) at 1M x 768 float32 over 256
lists, beside what a per-request filter costs without it: one JSON line.

    python tools/ivf_call_filter_bench.py [--rows 1000000] [--dim 768] [--nlist 256] [--k 10]

Rows and queries are bench.py's (the seeded device fill: corpus seed 12345, queries 42); the centroids are nlist of the rows.
Everything runs in one process, and a run that finds no GPU fails.  Before anything is timed, the three forms below are compared
bit for bit (labels, distances, last_search_stats) in every cell.  Every time is a host clock around a call that returns with the
device drained (the entry points synchronise before they answer), after two warm-up calls of the shape: three runs, the forms
alternating within a run, each the p50 of ten calls; the median of the three and their range.  The shader clock is read before and
after.

  cells   nq in {1, 64, 1024} x nprobe in {1, 8, 32} x visible in {100 %, 10 %, 1 %} (a random mask of that density)
    a     the bitmap search through device pointers, on a handle without a filter
    b     another handle under set_filter with the identical mask, searched through device pointers: the scan and the selection
          walk the same rows, so a - b is what the per-call compaction adds
    c     b plus the set_filter call in front of it: what a request that brings its own filter costs today
          (set_filter takes the byte mask from the host; the bitmap of `a` is in device memory already)
  Beside each cell the profiled slots of one call of `a` and one of `b` (a run of their own, profiling drains per batch): ms[1],
  the plan, which holds the compaction, and ms[2], the list scan.
  int8    1M x 64 int8 rows, 256 lists, 1024 queries x 32 probes, every row visible: the smallest row beside the 5 bytes a row that
          the compaction reads.  a, b and the slots.
  long    one query at one probe over a handle of 10 lists, every row visible and 10 %: one workgroup walks the whole list, the
          one nearest rows / 10 rows and the longest.  a, b and the slots.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import _lib, ivf  # noqa: E402

NQS = (1, 64, 1024)
NPROBES = (1, 8, 32)
VISIBLE = (100, 10, 1)


def p50_ms(fn, reps=10):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def clock_mhz(lib):
    try:
        return float(lib.lb_gpu_shader_clock_mhz(0, 2000))
    except Exception:
        return None


def summary(v):
    return {"ms": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


class Forms:
    """the three forms over one pair of handles: ha without a filter (a), hb under set_filter (b, c)"""

    def __init__(self, ha, hb, Q, k):
        self.ha, self.hb, self.Q, self.k = ha, hb, Q, k
        nq = Q.shape[0]
        self.D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        self.L = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        self.FD, self.FL = torch.empty_like(self.D), torch.empty_like(self.L)

    def set_mask(self, mask):
        self.mask = mask
        self.n = mask.size
        self.bits = torch.from_numpy(np.packbits(mask, bitorder="little")).cuda()
        self.hb.set_filter(mask)
        torch.cuda.synchronize()

    def a(self, nq, nprobe):
        return lambda: self.ha.search_device(nq, self.Q.data_ptr(), self.k, nprobe, self.D.data_ptr(), self.L.data_ptr(),
                                             d_bitmap=self.bits.data_ptr(), nbits=self.n)

    def b(self, nq, nprobe):
        return lambda: self.hb.search_device(nq, self.Q.data_ptr(), self.k, nprobe, self.FD.data_ptr(), self.FL.data_ptr())

    def c(self, nq, nprobe):
        b = self.b(nq, nprobe)

        def run():
            self.hb.set_filter(self.mask)
            b()
        return run

    def verify(self, nq, nprobe, ctx):
        self.a(nq, nprobe)()
        sa = self.ha.last_search_stats()
        self.b(nq, nprobe)()
        torch.cuda.synchronize()
        assert torch.equal(self.L[:nq], self.FL[:nq]) and torch.equal(self.D[:nq], self.FD[:nq]), ctx
        assert sa == self.hb.last_search_stats(), (ctx, sa, self.hb.last_search_stats())
        return sa

    def slots(self, nq, nprobe):
        """ms[1] (plan; with the compaction in `a`) and ms[2] (list scan) of one profiled call of each form"""
        out = {}
        for name, h, fn in (("a", self.ha, self.a(nq, nprobe)), ("b", self.hb, self.b(nq, nprobe))):
            h.set_profiling(True)
            fn()
            fn()
            t = h.last_timing()
            h.set_profiling(False)
            out[name] = {"plan_ms": t[1], "scan_ms": t[2], "select_ms": t[3]}
        return out

    def cell(self, nq, nprobe, forms=("a", "b", "c")):
        fns = {f: getattr(self, f)(nq, nprobe) for f in forms}
        for fn in fns.values():  # warm-up of the shape
            fn()
            fn()
        runs = {f: [] for f in forms}
        for _ in range(3):
            for f, fn in fns.items():
                runs[f].append(p50_ms(fn))
        out = {f: summary(v) for f, v in runs.items()}
        out["profiled"] = self.slots(nq, nprobe)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args()
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, d, k, nlist = a.rows, a.dim, a.k, a.nlist
    out = {"rows": n, "dim": d, "nlist": nlist, "k": k, "shader_clock_mhz_before": clock_mhz(lib)}
    X = torch.empty((n, d), dtype=torch.float32, device="cuda")
    Q = torch.empty((1024, d), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), X.numel(), 12345, 0, None))
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), Q.numel(), 42, 0, None))
    rng = np.random.default_rng(1)
    score = rng.random(n)  # row r is visible at p % iff score[r] < p / 100: nested masks
    torch.cuda.synchronize()

    def pair(cent, rows=X, cls=ivf.IVFFlat):
        hs = []
        for _ in range(2):
            h = cls(cent)
            h.add_device(rows.shape[0], rows.data_ptr())
            hs.append(h)
        return hs

    # ---- the table ---------------------------------------------------------------------------------------------------------
    cent = X[torch.from_numpy(np.sort(rng.permutation(n)[:nlist])).cuda()].cpu().numpy()
    ha, hb = pair(cent)
    sizes = ha.list_sizes()
    out["list_sizes"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max())}
    f = Forms(ha, hb, Q, k)
    table = {}
    for pct in VISIBLE:
        f.set_mask((score < pct / 100.0).astype(np.uint8))
        out[f"visible_rows_{pct}pct"] = int(f.mask.sum())
        for nq in NQS:
            for nprobe in NPROBES:
                st = f.verify(nq, nprobe, f"{pct} % visible, {nq} queries, {nprobe} probes")
                cell = f.cell(nq, nprobe)
                cell["rows_scanned"] = st[1]
                table[f"vis{pct}_q{nq}_nprobe{nprobe}"] = cell
                print(f"vis{pct}_q{nq}_nprobe{nprobe}", json.dumps(cell), file=sys.stderr, flush=True)
        assert ha.nvisible() == n  # the handle searched under bitmaps never had a filter
    out["cells"] = table
    t0 = time.perf_counter()
    hb.set_filter(f.mask)
    out["set_filter_ms_last_mask"] = (time.perf_counter() - t0) * 1e3
    ha.Close()
    hb.Close()

    # ---- the long list: ten lists, one query, one probe --------------------------------------------------------------------
    cent10 = X[torch.from_numpy(np.sort(rng.permutation(n)[:10])).cuda()].cpu().numpy()
    ha, hb = pair(cent10)
    sizes10 = ha.list_sizes()
    out["long_list_sizes"] = [int(s) for s in sizes10]
    assign10 = ha.assignments()
    # the query is a row of the list it is to probe (its own centroid is its nearest): the list nearest rows / 10, and the longest
    for name, l in (("long_list", int(np.argmin(np.abs(sizes10 - n // 10)))), ("longest_list", int(np.argmax(sizes10)))):
        f = Forms(ha, hb, X[int(np.flatnonzero(assign10 == l)[0])].reshape(1, d).clone(), k)
        for pct in (100, 10):
            f.set_mask((score < pct / 100.0).astype(np.uint8))
            st = f.verify(1, 1, f"{name}, {pct} % visible")
            assert pct != 100 or st[1] == sizes10[l], (st, int(sizes10[l]))
            cell = f.cell(1, 1, forms=("a", "b"))
            cell["list_rows"], cell["rows_scanned"] = int(sizes10[l]), st[1]
            out[f"{name}_vis{pct}"] = cell
    ha.Close()
    hb.Close()
    del X

    # ---- int8 rows of 64 bytes ---------------------------------------------------------------------------------------------
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    X8 = torch.randint(-128, 128, (n, 64), dtype=torch.int8, device="cuda", generator=g)
    Q8 = torch.randint(-128, 128, (1024, 64), dtype=torch.int8, device="cuda", generator=g)
    cent8 = X8[torch.from_numpy(np.sort(rng.permutation(n)[:nlist])).cuda()].cpu().numpy().astype(np.float32)
    ha, hb = pair(cent8, X8, ivf.IVFFlatInt8)
    f = Forms(ha, hb, Q8, k)
    f.set_mask(np.ones(n, np.uint8))
    st = f.verify(1024, 32, "int8 D = 64")
    cell = f.cell(1024, 32, forms=("a", "b"))
    cell["rows_scanned"] = st[1]
    out["int8_d64_q1024_nprobe32_vis100"] = cell
    ha.Close()
    hb.Close()
    out["shader_clock_mhz_after"] = clock_mhz(lib)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
