"""Removal and compaction of the IVF-Flat handle (lb_gpu_ivf_remove*, lb_gpu_ivf_compact) at 1M x 768 float32 over 256 lists: one
JSON line.

    python tools/ivf_remove_bench.py [--rows 1000000] [--dim 768] [--nlist 256] [--k 10]

Rows and queries are bench.py's (the seeded device fill: corpus seed 12345, queries 42); the centroids are nlist of the rows.
Everything runs in one process, and a run that finds no GPU fails.  Before anything is timed, the searches of every state (removed,
filtered, compacted) with every list probed are compared bit for bit with the flat index after the same removals.  Every time is a
host clock around a call that returns with the device drained (the entry points synchronise before they answer), after two warm-up
calls.  The shader clock is read before and after.

  1. remove_rows of 10,000 positions, and remove of 10,000 ids (the lookup over every row's id): the median of three calls after a
     warm-up call, each on rows that are still live;
  2. the single-query and the 1024-query search at nprobe 1, 8, 32 with 1 % and 10 % removed, on three handles side by side: one
     whose rows are removed, one under set_filter with the identical mask (the parent of this entry point cannot remove: the
     identical filter is the yardstick; both walk the same visible lists) and one untouched.  Three runs, the handles alternating
     within a run, each the p50 of ten calls: the median of the three and their range;
  3. compact at 10 % and 50 % removed beside what there was before: a fresh handle filled by add_device from a device buffer of
     the survivors, which assigns every row again.  The median of three fresh handles after a warm-up handle.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import _lib, gpu, ivf  # noqa: E402

NPROBES = (1, 8, 32)


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
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--check-queries", type=int, default=4)
    a = ap.parse_args()
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, d, k, nlist = a.rows, a.dim, a.k, a.nlist
    batch = min(10_000, n // 100)  # rows a removal call takes
    out = {"rows": n, "dim": d, "nlist": nlist, "k": k, "shader_clock_mhz_before": clock_mhz(lib)}
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
    torch.cuda.synchronize()

    def fresh(rows=X, with_ids=False):
        h = ivf.IVFFlat(cent)
        h.add_device(rows.shape[0], rows.data_ptr(), ids.data_ptr() if with_ids else None)
        return h

    def verify(h, flat, ctx):
        """every list probed: the flat index after the same removals, on a subsample of the queries"""
        nc = a.check_queries
        h.search_device(nc, Q.data_ptr(), k, nlist, D.data_ptr(), L.data_ptr())
        flat.search_device(nc, Q.data_ptr(), k, FD.data_ptr(), FL.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(L[:nc], FL[:nc]) and torch.equal(D[:nc], FD[:nc]), ctx

    def search(h, nq, nprobe):
        return lambda: h.search_device(nq, Q.data_ptr(), k, nprobe, D.data_ptr(), L.data_ptr())

    # ---- 1. removal of 10,000 rows -------------------------------------------------------------------------------------
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
        h.Close()

    # ---- 2. searches: untouched, filtered, removed ---------------------------------------------------------------------
    flat = gpu.Index(gpu.GPUConfig(DeviceID=0, Dimension=d))
    flat.add_device(n, X.data_ptr(), None)
    hb, hf, hr = fresh(), fresh(), fresh()
    verify(hb, flat, "before any removal")
    sizes = hb.list_sizes()
    out["list_sizes"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max())}
    for pct in (1, 10):
        gone = order[:n * pct // 100]
        live = np.ones(n, np.uint8)
        live[gone] = 0
        hf.set_filter(live)
        hr.remove_rows(gone)  # (the rows of the smaller set are removed already: ignored)
        flat.remove_rows(gone)
        assert hr.ndeleted() == gone.size and hr.nvisible() == hf.nvisible() == n - gone.size
        verify(hr, flat, f"{pct} % removed")
        verify(hf, flat, f"{pct} % filtered")
        cell = {}
        for nprobe in NPROBES:
            for nq in (1, 1024):
                runs = {"untouched": [], "filtered": [], "removed": []}
                for h in (hb, hf, hr):  # warm-up of the shape
                    search(h, nq, nprobe)()
                    search(h, nq, nprobe)()
                for _ in range(3):
                    for name, h in (("untouched", hb), ("filtered", hf), ("removed", hr)):
                        runs[name].append(p50_ms(search(h, nq, nprobe)))
                    assert hr.last_search_stats() == hf.last_search_stats()  # the same rows scanned
                cell[f"nprobe{nprobe}_q{nq}"] = {name: {"ms": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
                                                  for name, v in runs.items()}
        out[f"search_{pct}pct"] = cell
    old = hr.compact()
    assert np.array_equal(old, np.flatnonzero(live))
    flat.Compact()
    verify(hr, flat, "compacted")
    for h in (hb, hf, hr, flat):
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
        survivors = X.index_select(0, keep_t)  # (the second copy of the rows the fresh build needs; not timed)
        torch.cuda.synchronize()
        ts = []
        for rep in range(4):
            made = []
            ts.append(once_ms(lambda: made.append(fresh(survivors))))
            if rep == 0:  # the compacted handle is the fresh one
                assert np.array_equal(kept.assignments(), made[0].assignments()) and np.array_equal(kept.list_sizes(), made[0].list_sizes())
                for nprobe in (1, 32):
                    kept.search_device(64, Q.data_ptr(), k, nprobe, D.data_ptr(), L.data_ptr())
                    made[0].search_device(64, Q.data_ptr(), k, nprobe, FD.data_ptr(), FL.data_ptr())
                    torch.cuda.synchronize()
                    assert torch.equal(L[:64], FL[:64]) and torch.equal(D[:64], FD[:64]), (pct, nprobe)
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
