"""A row bitmap given with the search call on the flat index (lb_gpu_index_search_bitmap_device_ctx) at 1M x 768 float32, k = 100,
beside what a per-request filter costs without it: one JSON line.

    python tools/index_call_filter_bench.py [--rows 1000000] [--dim 768] [--k 100]

Rows and queries are bench.py's (the seeded device fill: corpus seed 12345, queries 42).  Everything runs in one process, and a run
that finds no GPU fails.  Before anything is timed, the three forms below are compared bit for bit (labels, distances) in every
cell.  Every time is a host clock around a call that returns with the device drained (the entry points synchronise before they
answer), after two warm-up calls of the shape: three runs, the forms alternating within a run, each the p50 of ten calls; the
median of the three and their range.  The shader clock is read before and after.

  cells   visible in {100 %, 10 %, 1 %} (a random mask of that density, nested) x nq in {1, 64, 1024}
    a     the bitmap search through device pointers, on an index without a filter
    b     a second index under set_filter with the identical mask, searched through device pointers: the search walks the same
          view, so a - b is the price of building the call's view
    c     b with the set_filter call in front of it: what a request that brings its own filter costs today
          (set_filter takes the byte mask from the host; the bitmap of `a` is in device memory already)
  Beside each cell one profiled call of `a` and one of `b` (a run of their own): the "select" class of last_timing, ms and
  launches, which in `a` holds the three launches that build the view, and the route both took.
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

NQS = (1, 64, 1024)
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
    """the three forms over one pair of indexes: ha without a filter (a), hb under set_filter (b, c)"""

    def __init__(self, ha, hb, Q, k):
        self.ha, self.hb, self.Q, self.k = ha, hb, Q, k
        nq = Q.shape[0]
        self.D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        self.L = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        self.FD, self.FL = torch.empty_like(self.D), torch.empty_like(self.L)

    def set_mask(self, mask):
        self.mask = mask
        self.n = mask.size
        self.bits = torch.from_numpy(gpu.pack_bitmap(mask)[0]).cuda()
        self.hb.set_filter(mask)
        torch.cuda.synchronize()

    def a(self, nq):
        return lambda: self.ha.search_device(nq, self.Q.data_ptr(), self.k, self.D.data_ptr(), self.L.data_ptr(),
                                             d_bitmap=self.bits.data_ptr(), nbits=self.n)

    def b(self, nq):
        return lambda: self.hb.search_device(nq, self.Q.data_ptr(), self.k, self.FD.data_ptr(), self.FL.data_ptr())

    def c(self, nq):
        b = self.b(nq)

        def run():
            self.hb.set_filter(self.mask)
            b()
        return run

    def verify(self, nq, ctx):
        self.a(nq)()
        self.b(nq)()
        torch.cuda.synchronize()
        assert torch.equal(self.L[:nq], self.FL[:nq]) and torch.equal(self.D[:nq], self.FD[:nq]), f"a != b: {ctx}"
        self.c(nq)()
        torch.cuda.synchronize()
        assert torch.equal(self.L[:nq], self.FL[:nq]) and torch.equal(self.D[:nq], self.FD[:nq]), f"a != c: {ctx}"

    def slots(self, nq):
        """the "select" class (ms, launches) and the whole device time of one profiled call of each form, and its route"""
        out = {}
        for name, h, fn in (("a", self.ha, self.a(nq)), ("b", self.hb, self.b(nq))):
            h.set_profiling(True)
            fn()
            fn()
            t = h.last_timing()
            h.set_profiling(False)
            out[name] = {"select_ms": t["select"][0], "select_launches": t["select"][1], "total_ms": t["total"][0],
                         "route": h.last_route[0] * 10 + h.last_route[1]}
        out["view_launches"] = out["a"]["select_launches"] - out["b"]["select_launches"]
        out["view_ms"] = out["a"]["select_ms"] - out["b"]["select_ms"]
        return out

    def cell(self, nq):
        fns = {f: getattr(self, f)(nq) for f in ("a", "b", "c")}
        for fn in fns.values():  # warm-up of the shape
            fn()
            fn()
        runs = {f: [] for f in fns}
        for _ in range(3):
            for f, fn in fns.items():
                runs[f].append(p50_ms(fn))
        out = {f: summary(v) for f, v in runs.items()}
        out["a_minus_b_ms"] = out["a"]["ms"] - out["b"]["ms"]
        out["a_over_c"] = out["a"]["ms"] / out["c"]["ms"]
        out["profiled"] = self.slots(nq)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    a = ap.parse_args()
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, d, k = a.rows, a.dim, a.k
    out = {"rows": n, "dim": d, "k": k, "shader_clock_mhz_before": clock_mhz(lib)}
    X = torch.empty((n, d), dtype=torch.float32, device="cuda")
    Q = torch.empty((max(NQS), d), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), X.numel(), 12345, 0, None))
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), Q.numel(), 42, 0, None))
    rng = np.random.default_rng(1)
    score = rng.random(n)  # row r is visible at p % iff score[r] < p / 100: nested masks
    torch.cuda.synchronize()
    hs = []
    for _ in range(2):
        h = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=d, Metric=0))
        h.add_device(n, X.data_ptr())
        hs.append(h)
    del X
    ha, hb = hs
    f = Forms(ha, hb, Q, k)
    table, loses = {}, []
    for pct in VISIBLE:
        f.set_mask((score < pct / 100.0).astype(np.uint8))
        out[f"visible_rows_{pct}pct"] = int(f.mask.sum())
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            hb.set_filter(f.mask)
            t.append((time.perf_counter() - t0) * 1e3)
        out[f"set_filter_ms_{pct}pct"] = summary(t)
        for nq in NQS:
            f.verify(nq, f"{pct} % visible, {nq} queries")
            cell = f.cell(nq)
            name = f"vis{pct}_q{nq}"
            table[name] = cell
            if cell["a"]["ms"] > cell["c"]["ms"]:
                loses.append(name)
            print(name, json.dumps(cell), file=sys.stderr, flush=True)
        assert ha.nvisible() == n  # the index searched under bitmaps never had a filter
    out["cells"] = table
    out["a_loses_to_c_in"] = loses
    ha.Close()
    hb.Close()
    out["shader_clock_mhz_after"] = clock_mhz(lib)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
