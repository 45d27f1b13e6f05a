"""Removal and compaction of the flat index (lb_gpu_index_remove*, lb_gpu_index_compact) at 1M x 768 float32: one JSON line.

    python tools/remove_bench.py [--rows 1000000] [--dim 768] [--k 10]

Rows and queries are bench.py's (the seeded device fill: corpus seed 12345, queries 42), everything runs in one process, and a run
that finds no GPU fails.  Before anything is timed, the searches of every state (removed, filtered, compacted) are compared bit
for bit with the oracle on a subsample of the queries.  Every time is a host clock around a call that returns with the device
drained (the entry points synchronise before they answer), after two warm-up calls: the median of three runs, each the p50 of
ten calls; one-shot calls (remove, compact, the rebuild) are the median of three fresh handles after a warm-up handle.

  1. remove of 10,000 labels, on an index without ids (positions) and on one with ids (the lookup over every row's id);
  2. the single-query p50 and the 1024-query batch at 1 % and 10 % removed, beside the same handle under set_filter with the
     identical mask (the same routes), before any removal, and after compact;
  3. compact at 10 % and 50 % removed: the call's time with the fp16 image on (the default: the image is rebuilt inside the
     call) and off, the bytes its gather moves (every survivor behind the first removed row is read and written twice: into the
     scratch and back) over the image-off time -- a lower bound of the gather's rate, the call also recomputes the norms --
     beside what there was before: a fresh handle filled by add_device from a device buffer of the survivors.
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
from oracle import oracle_c as oc  # noqa: E402


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


def once_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--check-queries", type=int, default=2)
    a = ap.parse_args()
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, d, k = a.rows, a.dim, a.k
    X = torch.empty((n, d), dtype=torch.float32, device="cuda")
    Q = torch.empty((1024, d), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), X.numel(), 12345, 0, None))
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), Q.numel(), 42, 0, None))
    D = torch.empty((1024, k), dtype=torch.float32, device="cuda")
    L = torch.empty((1024, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    Xh = oc.fill_uniform(n * d, 12345).reshape(n, d)
    Qh = oc.fill_uniform(1024 * d, 42).reshape(1024, d)
    ids = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 7
    rng = np.random.default_rng(1)
    order = rng.permutation(n).astype(np.int64)  # the first m entries are "the m removed rows": nested sets
    out = {"rows": n, "dim": d, "k": k}

    def fresh(with_ids=False, image=True):
        idx = gpu.Index(gpu.GPUConfig(DeviceID=0, Dimension=d))
        if not image:
            idx.set_f16_image(0)
        idx.add_device(n, X.data_ptr(), ids.data_ptr() if with_ids else None)
        return idx

    def verify(idx, live, Xs, ctx):
        """the searches of this state against the oracle, single query and batch, on a subsample"""
        nc = a.check_queries
        want = oc.search_batch(0, Qh[:nc], Xs, k, mask=live, nthreads=16)
        for nq in (1, 1024):
            idx.search_device(nq, Q.data_ptr(), k, D.data_ptr(), L.data_ptr())
            m = min(nq, nc)
            assert np.array_equal(L[:m].cpu().numpy(), want[0][:m]) and np.array_equal(D[:m].cpu().numpy(), want[1][:m]), ctx

    def search_times(idx):
        return {"q1_p50_ms": median_of_p50s(lambda: idx.search_device(1, Q.data_ptr(), k, D.data_ptr(), L.data_ptr())),
                "q1024_ms": median_of_p50s(lambda: idx.search_device(1024, Q.data_ptr(), k, D.data_ptr(), L.data_ptr()))}

    # ---- 1. remove of 10,000 labels --------------------------------------------------------------------------------
    for with_ids in (False, True):
        idx = fresh(with_ids)
        ts = []
        for rep in range(4):  # (the first is the warm-up; each takes 10,000 rows that are still live)
            rows = order[rep * 10_000:(rep + 1) * 10_000]
            labels = rows * 3 + 7 if with_ids else rows
            got = []
            ts.append(once_ms(lambda: got.append(idx.Remove(labels))))
            assert got[0] == 10_000
        out["remove_10000_ms_with_ids" if with_ids else "remove_10000_ms_positions"] = float(np.median(ts[1:]))
        idx.Close()

    # ---- 2. searches: before, filtered, removed, compacted ---------------------------------------------------------
    idx = fresh()
    verify(idx, np.ones(n, np.uint8), Xh, "before any removal")
    out["search_before"] = search_times(idx)
    for pct in (1, 10):
        gone = order[:n * pct // 100]
        live = np.ones(n, np.uint8)
        live[gone] = 0
        idx.set_filter(live)
        verify(idx, live, Xh, f"{pct} % filtered")
        out[f"search_filtered_{pct}pct"] = search_times(idx)
        idx.set_filter(None)
        idx.Remove(gone)  # (the rows of the smaller set are removed already: ignored)
        assert idx.ndeleted() == gone.size
        verify(idx, live, Xh, f"{pct} % removed")
        out[f"search_removed_{pct}pct"] = search_times(idx)
    keep = np.flatnonzero(live)
    assert np.array_equal(idx.Compact(), keep)
    verify(idx, np.ones(keep.size, np.uint8), Xh[keep], "compacted")
    out["search_compacted_10pct"] = search_times(idx)
    idx.Close()

    # ---- 3. compact beside the rebuild -----------------------------------------------------------------------------
    for pct in (10, 50):
        gone = order[:n * pct // 100]
        keep_t = torch.from_numpy(np.setdiff1d(np.arange(n), gone)).cuda()
        moved = int(keep_t.numel() - int(gone.min()))  # survivors behind the first removed row
        cell = {"survivors": int(keep_t.numel()), "gather_bytes": 4 * moved * d * 4}
        for image in (True, False):
            ts = []
            for rep in range(4):
                idx = fresh(image=image)
                idx.remove_rows(gone)
                ts.append(once_ms(idx.Compact))
                if rep == 0 and image:
                    live = np.ones(n, np.uint8)
                    live[gone] = 0
                    verify(idx, np.ones(int(live.sum()), np.uint8), Xh[np.flatnonzero(live)], f"compact {pct} %")
                idx.Close()
            cell["compact_ms_image_on" if image else "compact_ms_image_off"] = float(np.median(ts[1:]))
        cell["gather_tb_per_s_lower_bound"] = cell["gather_bytes"] / cell["compact_ms_image_off"] / 1e9
        survivors = X.index_select(0, keep_t)  # (the second copy of the corpus the rebuild needs; not timed)
        torch.cuda.synchronize()
        ts = []
        for rep in range(4):
            made = []

            def rebuild():
                r = gpu.Index(gpu.GPUConfig(DeviceID=0, Dimension=d))
                r.add_device(survivors.shape[0], survivors.data_ptr())
                made.append(r)

            ts.append(once_ms(rebuild))
            made[0].Close()
        cell["rebuild_ms"] = float(np.median(ts[1:]))
        cell["rebuild_extra_hbm_bytes"] = int(survivors.numel()) * 4
        cell["faster"] = "compact" if cell["compact_ms_image_on"] < cell["rebuild_ms"] else "rebuild"
        del survivors
        out[f"compact_{pct}pct"] = cell
    print(json.dumps(out))


if __name__ == "__main__":
    main()
