"""IVF-PQ index (exact ADC k-NN over the codes of the probed lists) against the flat ADC search of a PQ handle on the same codes:
one JSON line.

    python tools/ivfpq_bench.py [--rows 10000000] [--dim 768] [--m 96] [--nlist 1024] [--k 100]

Rows and queries come from the seeded device fill (uniform in [-0.5, 0.5)), the rows in pieces of --piece rows that are added
with add_device and never held together; the codebooks are config 4's of bench.py (the seeded fill, seed 7); the centroids are
nlist of the rows (evenly spaced).  The same codes go to a pq.PQEncoder.  Per cell (nq x nprobe): the median of three runs, each
the p50 of ten searches after a warm-up, through the device-pointer entry point by wall clock (the call returns when the results
are on the device); the HIP-event time of each step from one more, profiled, run (probes, plan, tables, scan, selection); rows
scanned and the scan's bytes (rows * (M + 4): a code row and its row number) over its time; recall@k against lb_gpu_pq_search
over the same codes, which is the full ADC ranking, not the exact f32 one; and that search's own p50 at the same nq, in the
same run.  Also: the add rate in rows/s and hbm_bytes against its per-row terms.  The shader clock is read before and after.  A
run that finds no GPU fails.

--residual builds a residual handle (lb_gpu_ivfpq_new_residual) beside the plain one, over the same rows, centroids and
codebooks, and searches both in every cell: the cell gains "residual": p50, the five step times (probes, plan, residual queries +
tables, scan, selection), rows scanned and the pairs (nq * nprobe) its scan ran over.

--clustered replaces the uniform fill: rows are centres[owner] + unit noise, centres spread * N(0, 1) (--spread, default 3), one
centre per list, queries drawn the same way; centroids and codebooks come from ivfpq.train over a sample of --train-rows rows
(the residual handle's codebooks from ivfpq.train(..., residual=True)); past ivf.train's 256 lists the centroids come from
ivf.train_coarse over the same sample and are handed to ivfpq.train, so --nlist goes up to 65,536.  The rows are also kept in an exact f32 gpu.Index, and every cell gains recall@k against its search of all rows ("recall_at_k_vs_exact_f32").

--refine C (with --clustered) adds the second stage to every cell, for the plain handle and, with --residual, the residual one:
the handle's search for C rows into device buffers, then lb_gpu_index_refine on the exact index's rows for k of them, on the same
stream.  The cell gains "refine": the p50 of the search for C, of the refine alone and of the two chained, and recall@k of the
refined result against the exact f32 search.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import _lib, gpu, ivf, ivfpq, pq  # noqa: E402


def p50_ms(fn, reps=10):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def median_of_p50s(fn, runs=3):
    fn()
    fn()
    return float(np.median([p50_ms(fn) for _ in range(runs)]))


def clock_mhz(lib):
    try:
        return float(lib.lb_gpu_shader_clock_mhz(0, 2000))
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--piece", type=int, default=1_000_000)
    ap.add_argument("--nprobe", type=int, nargs="*", default=[1, 8, 32, 1024])
    ap.add_argument("--nq", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--residual", action="store_true", help="also build and search a residual handle")
    ap.add_argument("--clustered", action="store_true", help="rows around one centre per list; trained centroids and codebooks")
    ap.add_argument("--spread", type=float, default=3.0)
    ap.add_argument("--train-rows", type=int, default=65536)
    ap.add_argument("--refine", type=int, default=0, metavar="C", help="with --clustered: refine a shortlist of C rows on the exact f32 rows")
    a = ap.parse_args()
    if a.refine and not a.clustered:
        ap.error("--refine needs --clustered (the exact f32 index)")
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, dim, M = a.rows, a.dim, a.m
    out = {"rows": n, "dim": dim, "m": M, "nlist": a.nlist, "k": a.k, "shader_clock_mhz_before": clock_mhz(lib)}

    out["residual"], out["clustered"] = a.residual, a.clustered
    rblob = None
    if a.clustered:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(12345)
        centres = a.spread * torch.randn((a.nlist, dim), generator=gen, device="cuda")

        def draw(cnt, dst):  # centres[owner] + unit noise
            owner = torch.randint(0, a.nlist, (cnt,), generator=gen, device="cuda")
            dst[:cnt].normal_(generator=gen)
            dst[:cnt] += centres[owner]

        sample = torch.empty((min(a.train_rows, n), dim), dtype=torch.float32, device="cuda")
        draw(sample.shape[0], sample)
        torch.cuda.synchronize()
        sample = sample.cpu().numpy()
        t0 = time.perf_counter()
        coarse = ivf.train_coarse(sample, a.nlist) if a.nlist > ivf.TRAIN_MAX_NLIST else None
        cent_np, blob = ivfpq.train(sample, a.nlist, M, centroids=coarse)
        if a.residual:
            _, rblob = ivfpq.train(sample, a.nlist, M, residual=True, centroids=coarse)
        out["train"] = {"rows": int(sample.shape[0]), "seconds": time.perf_counter() - t0, "spread": a.spread}
        del sample
    else:
        cb = torch.empty(M * 256 * (dim // M), dtype=torch.float32, device="cuda")
        _lib.check(lib.lb_gpu_fill_uniform_device(0, cb.data_ptr(), cb.numel(), 7, 0, None))
        torch.cuda.synchronize()
        blob = pq.serialize_codebooks(cb.cpu().numpy().reshape(M, 256, dim // M))
        # the centroids: rows 0, n / nlist, 2 n / nlist, ... of the same fill
        rows = torch.arange(a.nlist, dtype=torch.int64, device="cuda") * (n // a.nlist)
        cent = torch.empty((a.nlist, dim), dtype=torch.float32, device="cuda")
        _lib.check(lib.lb_gpu_fill_uniform_rows_device(0, cent.data_ptr(), rows.data_ptr(), a.nlist, dim, 12345, None))
        torch.cuda.synchronize()
        cent_np = cent.cpu().numpy()

        def draw(cnt, dst, r0=0, seed=12345):
            _lib.check(lib.lb_gpu_fill_uniform_device(0, dst.data_ptr(), cnt * dim, seed, r0 * dim, None))

    h = ivfpq.IVFPQ(blob, cent_np)
    h.reserve(n)
    hr = None
    if a.residual:  # the same rows, centroids and (unless trained) codebooks, encoded as residuals
        hr = ivfpq.IVFPQ(rblob or blob, cent_np, residual=True)
        hr.reserve(n)
    exact = None
    if a.clustered:  # the f32 rows themselves, for the recall
        exact = gpu.Index(gpu.GPUConfig(DeviceID=0, Dimension=dim))
        exact.reserve(n)
    buf = torch.empty((min(a.piece, n), dim), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    add_s = radd_s = 0.0
    for r0 in range(0, n, a.piece):
        cnt = min(a.piece, n - r0)
        if a.clustered:
            draw(cnt, buf)
        else:
            draw(cnt, buf, r0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.add_device(cnt, buf.data_ptr())
        add_s += time.perf_counter() - t0
        if hr is not None:
            t0 = time.perf_counter()
            hr.add_device(cnt, buf.data_ptr())
            radd_s += time.perf_counter() - t0
        if exact is not None:
            exact.add_device(cnt, buf.data_ptr())
    del buf
    sizes = h.list_sizes()
    out["add"] = {"seconds": add_s, "rows_per_s": n / add_s, "pieces": -(-n // a.piece)}
    if hr is not None:
        out["residual_add"] = {"seconds": radd_s, "rows_per_s": n / radd_s}
        out["residual_hbm_bytes"] = hr.hbm_bytes
    out["lists"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}
    per_row = 3 * M + 4 * 3  # the codes three times; assign and the two lists
    out["hbm_bytes"] = h.hbm_bytes
    out["hbm_bytes_per_row_terms"] = n * per_row
    out["hbm_bytes_beyond_rows"] = h.hbm_bytes - n * per_row  # codebooks, offsets, the coarse index

    enc = pq.PQEncoder(blob)
    enc.reserve(n)
    step = 1_000_000
    for r0 in range(0, n, step):
        enc.add_codes(h.codes(r0, min(step, n - r0)))

    nqmax = max(a.nq)
    Q = torch.empty((nqmax, dim), dtype=torch.float32, device="cuda")
    if a.clustered:
        draw(nqmax, Q)
    else:
        draw(nqmax, Q, 0, 42)
    D = torch.empty((nqmax, a.k), dtype=torch.float32, device="cuda")
    L = torch.empty((nqmax, a.k), dtype=torch.int64, device="cuda")
    FD = torch.empty((nqmax, a.k), dtype=torch.float32, device="cuda")
    FL = torch.empty((nqmax, a.k), dtype=torch.int64, device="cuda")
    if a.refine:
        SD = torch.empty((nqmax, a.refine), dtype=torch.float32, device="cuda")
        SL = torch.empty((nqmax, a.refine), dtype=torch.int64, device="cuda")

    def refined(handle, nq, nprobe, f32_truth):
        """the shortlist search, the refine and both chained: p50s and the refined recall"""
        short = lambda: handle.search_device(nq, Q.data_ptr(), a.refine, nprobe, SD.data_ptr(), SL.data_ptr())  # noqa: E731
        fine = lambda: exact.refine_device(nq, Q.data_ptr(), a.refine, SL.data_ptr(), a.k, D.data_ptr(), L.data_ptr())  # noqa: E731
        both = lambda: (short(), fine())  # noqa: E731
        short_ms = median_of_p50s(short)
        fine_ms = median_of_p50s(fine)
        both_ms = median_of_p50s(both)
        got = L[:nq].cpu().numpy()
        return {"c": a.refine, "shortlist_p50_ms": short_ms, "refine_p50_ms": fine_ms, "chained_p50_ms": both_ms,
                "recall_at_k_vs_exact_f32": float(np.mean([np.intersect1d(got[j], f32_truth[j]).size / a.k for j in range(nq)]))}

    torch.cuda.synchronize()
    cells = []
    for nq in a.nq:
        flat_ms = median_of_p50s(lambda: enc.search_device(nq, Q.data_ptr(), a.k, FD.data_ptr(), FL.data_ptr()))
        truth, truth_d = FL[:nq].cpu().numpy(), FD[:nq].cpu().numpy()
        if exact is not None:
            exact.search_device(nq, Q.data_ptr(), a.k, FD.data_ptr(), FL.data_ptr())
            torch.cuda.synchronize()
            f32_truth = FL[:nq].cpu().numpy()
        for nprobe in a.nprobe:
            run = lambda: h.search_device(nq, Q.data_ptr(), a.k, nprobe, D.data_ptr(), L.data_ptr())  # noqa: E731
            ms = median_of_p50s(run)
            h.set_profiling(True)
            run()
            h.set_profiling(False)
            steps = h.last_timing()
            st = h.last_search_stats()
            got = L[:nq].cpu().numpy()
            recall = float(np.mean([np.intersect1d(got[j], truth[j]).size / a.k for j in range(nq)]))
            cell = {"nq": nq, "nprobe": nprobe, "p50_ms": ms, "flat_adc_p50_ms": flat_ms,
                    "probes_ms": steps[0], "plan_ms": steps[1], "tables_ms": steps[2], "scan_ms": steps[3], "select_ms": steps[4],
                    "rows_scanned": st[1], "max_rows_per_query": st[2], "selected_from_lds": st[3],
                    "scan_bytes": st[1] * (M + 4), "scan_gb_per_s": st[1] * (M + 4) / max(steps[3], 1e-6) / 1e6,
                    "recall_at_k_vs_full_adc": recall}
            if nprobe >= a.nlist:  # every list probed: the flat ADC search's own result, bit for bit
                cell["equals_flat_adc"] = bool(np.array_equal(got, truth) and np.array_equal(D[:nq].cpu().numpy(), truth_d))
            if exact is not None:
                cell["recall_at_k_vs_exact_f32"] = float(np.mean([np.intersect1d(got[j], f32_truth[j]).size / a.k for j in range(nq)]))
            if a.refine:
                cell["refine"] = refined(h, nq, nprobe, f32_truth)
            if hr is not None:
                rrun = lambda: hr.search_device(nq, Q.data_ptr(), a.k, nprobe, D.data_ptr(), L.data_ptr())  # noqa: E731
                rms = median_of_p50s(rrun)
                hr.set_profiling(True)
                rrun()
                hr.set_profiling(False)
                rsteps = hr.last_timing()
                rst = hr.last_search_stats()
                rgot = L[:nq].cpu().numpy()
                pairs = nq * min(nprobe, a.nlist)
                res = {"p50_ms": rms, "probes_ms": rsteps[0], "plan_ms": rsteps[1], "residual_tables_ms": rsteps[2], "scan_ms": rsteps[3],
                       "select_ms": rsteps[4], "rows_scanned": rst[1], "pairs": pairs, "table_bytes": pairs * M * 1024,
                       "scan_gb_per_s": (rst[1] * (M + 4) + pairs * M * 1024) / max(rsteps[3], 1e-6) / 1e6}
                if exact is not None:
                    res["recall_at_k_vs_exact_f32"] = float(np.mean([np.intersect1d(rgot[j], f32_truth[j]).size / a.k for j in range(nq)]))
                if a.refine:
                    res["refine"] = refined(hr, nq, nprobe, f32_truth)
                cell["residual"] = res
            cells.append(cell)
    out["cells"] = cells
    out["shader_clock_mhz_after"] = clock_mhz(lib)
    print(json.dumps(out))
    enc.Close()
    h.Close()
    if hr is not None:
        hr.Close()
    if exact is not None:
        exact.Close()


if __name__ == "__main__":
    main()
