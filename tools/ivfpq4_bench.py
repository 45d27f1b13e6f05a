"""IVF-PQ4 handles (packed 4-bit codes, ivfpq4.IVFPQ4) beside the K = 256 IVF-PQ handles (ivfpq.IVFPQ) over the same rows, in one
process: one JSON line.

    python tools/ivfpq4_bench.py [--rows 10000000] [--dim 768] [--m 96] [--nlist 1024] [--k 100] [--out FILE]

Rows and queries come from the seeded device fill (uniform in [-0.5, 0.5)), the rows in pieces of --piece rows that are added with
add_device to all four handles (plain and residual, K = 16 and K = 256) and never held together; the codebooks are the seeded
fill too (seed 7, the first 16 centroids of each subspace for K = 16); the centroids are nlist of the rows, evenly spaced.
Before anything is timed every cell's result is checked against the same handle's answer with every list probed: a row's
distance does not depend on which lists are probed, so the j-th distance is at least the every-list j-th and a label the two
share has the same distance, bit for bit.  Per cell (nq x nprobe) and handle: the median of three runs, each the p50 of ten
searches after a warm-up, through the device-pointer entry point by wall clock (the call returns when the results are on the
device), alternating the K = 16 and the K = 256 handle; the HIP-event times of the table and scan steps from one more,
profiled, run; and the ratio of the K = 256 p50 to the K = 16 one.  Also hbm_bytes of all four and the shader clock before and
after.  A run that finds no GPU fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import _lib, ivfpq, ivfpq4, pq  # noqa: E402


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


def check_against_every_list(lab, dist, all_lab, all_dist, what):
    """a cell's (labels, distances) against the same handle's answer with every list probed"""
    assert (np.diff(dist, axis=1) >= 0).all(), f"{what}: distances do not ascend"
    assert (dist >= all_dist).all(), f"{what}: a distance below the every-list answer's at the same rank"
    for j in range(lab.shape[0]):
        shared, a, b = np.intersect1d(lab[j][lab[j] >= 0], all_lab[j], return_indices=True)
        assert np.array_equal(dist[j][lab[j] >= 0][a], all_dist[j][b]), f"{what}: query {j}: a shared row's distance differs"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--piece", type=int, default=1_000_000)
    ap.add_argument("--nprobe", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--nq", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, dim, M = a.rows, a.dim, a.m
    out = {"rows": n, "dim": dim, "m": M, "nlist": a.nlist, "k": a.k, "shader_clock_mhz_before": clock_mhz(lib)}

    cb = torch.empty(M * 256 * (dim // M), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, cb.data_ptr(), cb.numel(), 7, 0, None))
    torch.cuda.synchronize()
    cb = cb.cpu().numpy().reshape(M, 256, dim // M)
    blobs = {256: pq.serialize_codebooks(cb), 16: pq.serialize_codebooks(np.ascontiguousarray(cb[:, :16]))}
    rows = torch.arange(a.nlist, dtype=torch.int64, device="cuda") * (n // a.nlist)
    cent = torch.empty((a.nlist, dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_rows_device(0, cent.data_ptr(), rows.data_ptr(), a.nlist, dim, 12345, None))
    torch.cuda.synchronize()
    cent = cent.cpu().numpy()

    # handles[(K, residual)]
    handles = {(K, r): (ivfpq4.IVFPQ4 if K == 16 else ivfpq.IVFPQ)(blobs[K], cent, residual=r) for K in (16, 256) for r in (False, True)}
    add_s = dict.fromkeys(handles, 0.0)
    for h in handles.values():
        h.reserve(n)
    buf = torch.empty((min(a.piece, n), dim), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, a.piece):
        cnt = min(a.piece, n - r0)
        _lib.check(lib.lb_gpu_fill_uniform_device(0, buf.data_ptr(), cnt * dim, 12345, r0 * dim, None))
        torch.cuda.synchronize()
        for key, h in handles.items():
            t0 = time.perf_counter()
            h.add_device(cnt, buf.data_ptr())
            add_s[key] += time.perf_counter() - t0
    del buf
    name = lambda K, r: f"k{K}_{'residual' if r else 'plain'}"  # noqa: E731
    out["hbm_bytes"] = {name(*key): h.hbm_bytes for key, h in handles.items()}
    out["add_rows_per_s"] = {name(*key): n / add_s[key] for key in handles}
    sizes = handles[(16, False)].list_sizes()
    out["lists"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}

    nqmax = max(a.nq)
    Q = torch.empty((nqmax, dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), nqmax * dim, 42, 0, None))
    D = torch.empty((nqmax, a.k), dtype=torch.float32, device="cuda")
    L = torch.empty((nqmax, a.k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def search(h, nq, nprobe):
        h.search_device(nq, Q.data_ptr(), a.k, nprobe, D.data_ptr(), L.data_ptr())

    # every cell of the K = 16 handles against their own every-list answers, before anything is timed
    for r in (False, True):
        h = handles[(16, r)]
        search(h, nqmax, a.nlist)
        all_lab, all_dist = L.cpu().numpy(), D.cpu().numpy()
        for nq in a.nq:
            for nprobe in a.nprobe:
                search(h, nq, nprobe)
                check_against_every_list(L[:nq].cpu().numpy(), D[:nq].cpu().numpy(), all_lab[:nq], all_dist[:nq],
                                         f"{name(16, r)} nq {nq} nprobe {nprobe}")
    out["checked_against_every_list"] = True

    cells = []
    for r in (False, True):
        for nq in a.nq:
            for nprobe in a.nprobe:
                cell = {"residual": r, "nq": nq, "nprobe": nprobe}
                runs = {K: (lambda h=handles[(K, r)]: search(h, nq, nprobe)) for K in (16, 256)}
                p50s = {16: [], 256: []}
                for K in (16, 256):  # warm-up
                    runs[K]()
                    runs[K]()
                for _ in range(3):  # alternating the two handles
                    for K in (16, 256):
                        p50s[K].append(p50_ms(runs[K]))
                for K in (16, 256):
                    h = handles[(K, r)]
                    h.set_profiling(True)
                    runs[K]()
                    h.set_profiling(False)
                    steps = h.last_timing()
                    cell[f"k{K}"] = {"p50_ms": float(np.median(p50s[K])), "p50_runs_ms": p50s[K], "tables_ms": steps[2], "scan_ms": steps[3],
                                     "select_ms": steps[4], "rows_scanned": h.last_search_stats()[1]}
                cell["k256_over_k16"] = cell["k256"]["p50_ms"] / cell["k16"]["p50_ms"]
                cells.append(cell)
    out["cells"] = cells
    out["shader_clock_mhz_after"] = clock_mhz(lib)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for h in handles.values():
        h.Close()


if __name__ == "__main__":
    main()
