"""Removal and compaction of the code handles that can forget rows (lb_gpu_ivfpq_* plain and residual, lb_gpu_ivfsq8_*
_remove*, _compact) at the shapes those handles' own bench tools use: one JSON line per run, one handle per process.

    python tools/ivf_code_remove_bench.py --index ivfpq [--residual] [--rows 10000000] [--dim 768] [--m 96] [--nlist 1024] [--k 10]
    python tools/ivf_code_remove_bench.py --index ivfsq8 [--rows 1000000] [--dim 768] [--nlist 256]

Rows and queries are bench.py's (the seeded device fill: corpus seed 12345, queries 42, uniform in [-0.5, 0.5)); the centroids are
nlist of the rows; the codebooks are the seeded fill of tools/ivfpq_bench.py (seed 7), the SQ8 bounds -0.5 / 0.5.  A run that finds
no GPU fails.  Before anything is timed, the searches of every state (removed, filtered, compacted) are compared bit for bit: with
every list probed against the flat code handle (pq / sq8) over the same codes under set_filter(live); a residual handle, whose
distances no flat handle has, against the same handle under the identical filter, and after compaction against a fresh handle of
the survivors' vectors.  Every time is a host clock around a call that returns with the device drained, after warm-up calls.  The
shader clock is read before and after.

  1. remove_rows of 10,000 positions and remove of 10,000 ids (the lookup over every row's id), beside one set_filter call on the
     same handle: the median of three calls after a warm-up call, each removal on rows that are still live;
  2. the single-query and the 1024-query search at nprobe 1, 8, 32 with 1 % and 10 % removed, on four handles side by side: one
     whose rows are removed, one under set_filter with the identical mask (the parent of these entry points cannot remove: the
     identical filter is the yardstick; both walk the same visible lists), a twin of that filtered handle (a second handle
     built and filtered in the same way: what two handles in the same state differ by) and one untouched.  Two runs, the handles
     alternating within a run, each the p50 of ten calls: both runs of every cell are reported, so the filtered cell's own
     run-to-run spread and the twin's distance stand beside the difference between removed and filtered;
  3. compact at 10 % and 50 % removed beside what there was before: a fresh handle filled by add_device from a second device buffer
     of the survivors' vectors, which assigns and encodes every row again.  The median of three after a warm-up.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import _lib, ivfpq, ivfsq8, pq, sq8  # noqa: E402

NPROBES = (1, 8, 32)
DEFAULTS = {"ivfpq": (10_000_000, 1024), "ivfsq8": (1_000_000, 256)}


def p50_ms(fn, reps=10):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def once_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def clock_mhz(lib):
    try:
        return float(lib.lb_gpu_shader_clock_mhz(0, 2000))
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", choices=sorted(DEFAULTS), required=True)
    ap.add_argument("--residual", action="store_true", help="ivfpq: a residual handle (lb_gpu_ivfpq_new_residual)")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--nlist", type=int, default=0)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--check-queries", type=int, default=4)
    a = ap.parse_args()
    if a.residual and a.index != "ivfpq":
        ap.error("--residual goes with --index ivfpq")
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, nlist = a.rows or DEFAULTS[a.index][0], a.nlist or DEFAULTS[a.index][1]
    d, k = a.dim, a.k
    batch = min(10_000, n // 100)  # rows a removal call takes
    out = {"index": a.index, "residual": a.residual, "rows": n, "dim": d, "nlist": nlist, "k": k, "shader_clock_mhz_before": clock_mhz(lib)}
    X = torch.empty((n, d), dtype=torch.float32, device="cuda")
    Q = torch.empty((1024, d), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), X.numel(), 12345, 0, None))
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), Q.numel(), 42, 0, None))
    D = torch.empty((1024, k), dtype=torch.float32, device="cuda")
    L = torch.empty((1024, k), dtype=torch.int64, device="cuda")
    FD, FL = torch.empty_like(D), torch.empty_like(L)
    ids = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 7
    rng = np.random.default_rng(1)
    order = rng.permutation(n).astype(np.int64)  # the first m entries are "the m removed rows": nested sets
    cent = X[torch.from_numpy(np.sort(rng.permutation(n)[:nlist])).cuda()].cpu().numpy()
    blob = None
    if a.index == "ivfpq":
        out["m"] = a.m
        cb = torch.empty(a.m * 256 * (d // a.m), dtype=torch.float32, device="cuda")
        _lib.check(lib.lb_gpu_fill_uniform_device(0, cb.data_ptr(), cb.numel(), 7, 0, None))
        torch.cuda.synchronize()
        blob = pq.serialize_codebooks(cb.cpu().numpy().reshape(a.m, 256, d // a.m))
    bounds = (np.full(d, -0.5, np.float32), np.full(d, 0.5, np.float32))
    torch.cuda.synchronize()

    def fresh(rows=X, with_ids=False):
        if a.index == "ivfpq":
            h = ivfpq.IVFPQ(blob, cent, residual=a.residual)
        else:
            h = ivfsq8.IVFSQ8(bounds[0], bounds[1], cent)
        h.add_device(rows.shape[0], rows.data_ptr(), ids.data_ptr() if with_ids else None)
        return h

    def flat_codes():
        """the flat code handle over the same vectors: the same codes.  None for a residual handle"""
        if a.residual:
            return None
        if a.index == "ivfpq":
            enc = pq.PQEncoder(blob)
        else:
            enc = sq8.SQ8Encoder(d)
            enc.set_bounds(*bounds)
        enc.add_vectors_device(n, X.data_ptr())
        return enc

    def same(h, other, nprobe, ctx, nc=None):
        """two IVF handles answer alike, bit for bit"""
        nc = nc or a.check_queries
        h.search_device(nc, Q.data_ptr(), k, nprobe, D.data_ptr(), L.data_ptr())
        other.search_device(nc, Q.data_ptr(), k, nprobe, FD.data_ptr(), FL.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(L[:nc], FL[:nc]) and torch.equal(D[:nc], FD[:nc]), ctx

    def verify(h, flat, ctx):
        """every list probed: the flat code handle under the same mask, on a subsample of the queries"""
        if flat is None:
            return
        nc = a.check_queries
        h.search_device(nc, Q.data_ptr(), k, nlist, D.data_ptr(), L.data_ptr())
        flat.search_device(nc, Q.data_ptr(), k, FD.data_ptr(), FL.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(L[:nc], FL[:nc]) and torch.equal(D[:nc], FD[:nc]), ctx

    def search(h, nq, nprobe):
        return lambda: h.search_device(nq, Q.data_ptr(), k, nprobe, D.data_ptr(), L.data_ptr())

    # ---- 1. removal of 10,000 rows, beside one set_filter call -----------------------------------------------------------
    for with_ids in (False, True):
        h = fresh(with_ids=with_ids)
        ts = []
        for rep in range(4):  # (the first is the warm-up; each takes rows that are still live)
            rows = order[rep * batch:(rep + 1) * batch]
            got = []
            call = (lambda: got.append(h.remove(rows * 3 + 7))) if with_ids else (lambda: got.append(h.remove_rows(rows)))
            ts.append(once_ms(call))
            assert got[0] == batch
        out["remove_ids_ms" if with_ids else "remove_rows_ms"] = float(np.median(ts[1:]))
        out["removal_batch"] = batch
        if not with_ids:
            live = np.ones(n, np.uint8)
            live[order[:4 * batch]] = 0
            ts = [once_ms(lambda: h.set_filter(live)) for _ in range(4)]
            out["set_filter_ms"] = float(np.median(ts[1:]))
        h.Close()

    # ---- 2. searches: untouched, filtered, removed ---------------------------------------------------------------------
    flat = flat_codes()
    hb, hf, ht, hr = fresh(), fresh(), fresh(), fresh()
    verify(hb, flat, "before any removal")
    sizes = hb.list_sizes()
    out["list_sizes"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max())}
    for pct in (1, 10):
        gone = order[:n * pct // 100]
        live = np.ones(n, np.uint8)
        live[gone] = 0
        hf.set_filter(live)
        ht.set_filter(live)
        hr.remove_rows(gone)  # (the rows of the smaller set are removed already: ignored)
        if flat is not None:
            flat.set_filter(live)
        assert hr.ndeleted() == gone.size and hr.nvisible() == hf.nvisible() == n - gone.size
        verify(hr, flat, f"{pct} % removed")
        verify(hf, flat, f"{pct} % filtered")
        for nprobe in NPROBES:
            same(hr, hf, nprobe, f"{pct} % removed against the identical filter, nprobe {nprobe}", nc=64)
        cell = {}
        for nprobe in NPROBES:
            for nq in (1, 1024):
                runs = {"untouched": [], "filtered": [], "filtered_twin": [], "removed": []}
                for h in (hb, hf, ht, hr):  # warm-up of the shape
                    search(h, nq, nprobe)()
                    search(h, nq, nprobe)()
                for _ in range(2):
                    for name, h in (("untouched", hb), ("filtered", hf), ("filtered_twin", ht), ("removed", hr)):
                        runs[name].append(p50_ms(search(h, nq, nprobe)))
                    assert hr.last_search_stats() == hf.last_search_stats()  # the same rows scanned
                f, r, t = runs["filtered"], runs["removed"], runs["filtered_twin"]
                cell[f"nprobe{nprobe}_q{nq}"] = {
                    **{name: {"ms": float(np.mean(v)), "runs": [float(x) for x in v]} for name, v in runs.items()},
                    "removed_over_filtered_pct": float((np.mean(r) / np.mean(f) - 1) * 100),
                    "twin_over_filtered_pct": float((np.mean(t) / np.mean(f) - 1) * 100),
                    "filtered_spread_pct": float(abs(f[0] - f[1]) / np.mean(f) * 100)}
        out[f"search_{pct}pct"] = cell
    old = hr.compact()
    assert np.array_equal(old, np.flatnonzero(live))
    assert hr.nvisible() == hf.nvisible()
    if flat is not None:  # (the flat code handles do not compact: the compacted handle answers in the new positions)
        nc = a.check_queries
        hr.search_device(nc, Q.data_ptr(), k, nlist, D.data_ptr(), L.data_ptr())
        flat.search_device(nc, Q.data_ptr(), k, FD.data_ptr(), FL.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(old[L[:nc].cpu().numpy()], FL[:nc].cpu().numpy()) and torch.equal(D[:nc], FD[:nc]), "compacted"
        flat.Close()
    for h in (hb, hf, ht, hr):
        h.Close()

    # ---- 3. compact beside the fresh build -----------------------------------------------------------------------------
    for pct in (10, 50):
        gone = order[:n * pct // 100]
        keep_t = torch.from_numpy(np.setdiff1d(np.arange(n), gone)).cuda()
        cell = {"survivors": int(keep_t.numel())}
        ts = []
        for rep in range(4):
            h = fresh()
            h.remove_rows(gone)
            ts.append(once_ms(h.compact))
            if rep == 0:
                kept = h
            else:
                h.Close()
        cell["compact_ms"] = float(np.median(ts[1:]))
        cell["compact_ms_min_max"] = [float(min(ts[1:])), float(max(ts[1:]))]
        survivors = X.index_select(0, keep_t)  # (the second copy of the vectors the fresh build needs; not timed)
        torch.cuda.synchronize()
        ts = []
        for rep in range(4):
            made = []
            ts.append(once_ms(lambda: made.append(fresh(survivors))))
            if rep == 0:  # the compacted handle is the fresh one: nothing needed encoding again
                assert np.array_equal(kept.assignments(), made[0].assignments()) and np.array_equal(kept.list_sizes(), made[0].list_sizes())
                step = 1_000_000
                for r0 in range(0, kept.ntotal, step):
                    assert np.array_equal(kept.codes(r0, min(step, kept.ntotal - r0)), made[0].codes(r0, min(step, kept.ntotal - r0))), (pct, r0)
                for nprobe in (1, 32):
                    same(kept, made[0], nprobe, f"compacted against fresh, {pct} % nprobe {nprobe}", nc=64)
                kept.Close()
            made[0].Close()
        cell["fresh_build_ms"] = float(np.median(ts[1:]))
        cell["fresh_build_ms_min_max"] = [float(min(ts[1:])), float(max(ts[1:]))]
        cell["fresh_build_extra_hbm_bytes"] = int(survivors.numel()) * 4
        cell["faster"] = "compact" if cell["compact_ms"] < cell["fresh_build_ms"] else "fresh build"
        del survivors
        out[f"compact_{pct}pct"] = cell
    out["shader_clock_mhz_after"] = clock_mhz(lib)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
