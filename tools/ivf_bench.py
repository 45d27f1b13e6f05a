"""IVF-Flat index (exact k-NN over the probed lists) against the brute-force f32 index on the same rows: one JSON line.

    python tools/ivf_bench.py [--rows 1000000] [--dim 768] [--nlist 256] [--k 100]

Rows and queries come from the seeded device fill (uniform in [-0.5, 0.5)); the centroids are nlist of the rows (ivf.train with
max_iter = 0 returns its init rows).  Per cell (nprobe x nq): the p50 of the whole search through the device-pointer entry point
as the median of three wall-clock runs after a warm-up (the call returns when the results are on the device); the HIP-event time
of each step from one more, profiled, run (probes, plan, list scan, selection); rows and bytes scanned (rows * dim * 4); the
scan pass's bytes per second and its share of 8 TB/s; recall@k against lb_gpu_index_search on an f32 index with the same rows;
and that index's own p50 for the same nq, in the same run.  Also: the add rate in rows/s, and one ivf.train(nlist = 256,
max_iter = 1) on 100k rows with its E-step time.  The shader clock is read before and after.  A run that finds no GPU fails.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import _lib, gpu, ivf  # noqa: E402

HBM_BYTES_PER_S = 8e12


def p50_ms(fn, reps=3):
    fn()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nprobe", type=int, nargs="*", default=[1, 8, 32, 256])
    ap.add_argument("--nq", type=int, nargs="*", default=[1, 8, 64, 1024])
    ap.add_argument("--train-rows", type=int, default=100_000)
    a = ap.parse_args()
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    out = {"rows": a.rows, "dim": a.dim, "nlist": a.nlist, "k": a.k, "shader_clock_mhz_before": clock_mhz(lib)}
    X = torch.empty((a.rows, a.dim), dtype=torch.float32, device="cuda")
    nqmax = max(a.nq)
    Q = torch.empty((nqmax, a.dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), a.rows * a.dim, 1, 0, None))
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), nqmax * a.dim, 2, 0, None))
    torch.cuda.synchronize()

    # one E-step of the wide-row k-means (km_estep_generic_kernel at sub = dim), never measured before
    tr = min(a.train_rows, a.rows)
    t0 = time.perf_counter()
    ivf.train_device(tr, X.data_ptr(), a.dim, min(a.nlist, 256), max_iter=1)
    wall_ms = (time.perf_counter() - t0) * 1e3
    ms3 = (C.c_float * 3)()
    lib.lb_gpu_pq_train_last_timing(ms3)
    out["train_1_iter"] = {"rows": tr, "nlist": min(a.nlist, 256), "wall_ms": wall_ms,
                           "estep_ms": float(ms3[0]), "order_ms": float(ms3[1]), "mstep_ms": float(ms3[2])}

    cent = ivf.train_device(a.rows, X.data_ptr(), a.dim, a.nlist, max_iter=0)  # nlist of the rows
    h = ivf.IVFFlat(cent)
    h.reserve(a.rows)
    t0 = time.perf_counter()
    h.add_device(a.rows, X.data_ptr())
    add_s = time.perf_counter() - t0
    sizes = h.list_sizes()
    out["add"] = {"seconds": add_s, "rows_per_s": a.rows / add_s}
    out["lists"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}
    out["hbm_bytes"] = h.hbm_bytes

    flat = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=a.dim, Metric=0))
    flat.set_order(0)
    flat.reserve(a.rows)
    flat.add_device(a.rows, X.data_ptr())
    D = torch.empty((nqmax, a.k), dtype=torch.float32, device="cuda")
    L = torch.empty((nqmax, a.k), dtype=torch.int64, device="cuda")
    FD = torch.empty((nqmax, a.k), dtype=torch.float32, device="cuda")
    FL = torch.empty((nqmax, a.k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cells = []
    for nq in a.nq:
        flat_ms = p50_ms(lambda: flat.search_device(nq, Q.data_ptr(), a.k, FD.data_ptr(), FL.data_ptr()))
        truth = FL[:nq].cpu().numpy()
        for nprobe in a.nprobe:
            run = lambda: h.search_device(nq, Q.data_ptr(), a.k, nprobe, D.data_ptr(), L.data_ptr())  # noqa: E731
            ms = p50_ms(run)
            h.set_profiling(True)
            run()
            h.set_profiling(False)
            steps = h.last_timing()
            st = h.last_search_stats()
            got = L[:nq].cpu().numpy()
            recall = float(np.mean([np.intersect1d(got[j], truth[j]).size / a.k for j in range(nq)]))
            scan_bytes = st[1] * a.dim * 4
            cells.append({"nq": nq, "nprobe": nprobe, "p50_ms": ms, "flat_p50_ms": flat_ms,
                          "probes_ms": steps[0], "plan_ms": steps[1], "scan_ms": steps[2], "select_ms": steps[3],
                          "rows_scanned": st[1], "max_rows_per_query": st[2], "selected_from_lds": st[3], "bytes_scanned": scan_bytes,
                          "scan_tb_per_s": scan_bytes / max(steps[2], 1e-6) / 1e9,
                          "scan_share_of_8tb": scan_bytes / max(steps[2], 1e-6) * 1e3 / HBM_BYTES_PER_S,
                          "recall_at_k": recall})
    out["cells"] = cells
    out["shader_clock_mhz_after"] = clock_mhz(lib)
    print(json.dumps(out))
    flat.Close()
    h.Close()


if __name__ == "__main__":
    main()
