"""IVF-SQ8 index (exact integer k-NN over the codes of the probed lists) against the flat search of an SQ8 handle on the same
codes: one JSON line.

    python tools/ivfsq8_bench.py [--rows 1000000] [--dim 768] [--nlist 256] [--k 100]

Rows and queries come from the seeded device fill (uniform in [-0.5, 0.5)), the rows in pieces of --piece rows that are added
with add_device and never held together; the bounds are -0.5 / 0.5 in every dimension; the centroids are nlist of the rows
(evenly spaced).  The same vectors go to an sq8.SQ8Encoder with the same bounds, so it holds the same codes.  Per cell
(nq x nprobe): the median of three runs, each the p50 of ten searches after a warm-up, through the device-pointer entry point by
wall clock (the call returns when the results are on the device); the HIP-event time of each step as the median of three more,
profiled, runs (probes, plan, the queries' codes, scan, selection); rows scanned and the scan's bytes (rows * stride for the
codes, nothing for norms, which are not kept, plus 8 per key written) over its time; recall@k against lb_gpu_sq8_search over the
same codes, which is the full integer ranking, not the exact f32 one; and that search's own p50 at the same nq, in the same run.
Also: the add rate in rows/s and hbm_bytes against its per-row terms.  The shader clock is read before and after.  A run that
finds no GPU fails.

--clustered replaces the uniform fill: rows are centres[owner] + unit noise, centres spread * N(0, 1) (--spread, default 3), one
centre per list, queries drawn the same way (tools/ivfpq_bench.py --clustered's data: the same generator and seed); centroids and
bounds come from ivfsq8.train over a sample of --train-rows rows; past ivf.train's 256 lists the centroids come from
ivf.train_coarse over the same sample and are handed to it, so --nlist goes up to 65,536.  The rows are also kept in an exact f32 gpu.Index, and every cell gains recall@k against its search of all rows ("recall_at_k_vs_exact_f32").

--refine C (with --clustered) adds the second stage to every cell: the handle's search for C rows into device buffers, then
lb_gpu_index_refine on the exact index's rows for k of them, on the same stream.  The cell gains "refine": the p50 of the search
for C, of the refine alone and of the two chained, and recall@k of the refined result against the exact f32 search.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from longbow_amd import _lib, gpu, ivf, ivfsq8, sq8  # noqa: E402

STEPS = ("probes_ms", "plan_ms", "codes_ms", "scan_ms", "select_ms")


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
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--piece", type=int, default=1_000_000)
    ap.add_argument("--nprobe", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--nq", type=int, nargs="*", default=[1, 8, 64, 1024])
    ap.add_argument("--clustered", action="store_true", help="rows around one centre per list; trained centroids and bounds")
    ap.add_argument("--spread", type=float, default=3.0)
    ap.add_argument("--train-rows", type=int, default=65536)
    ap.add_argument("--refine", type=int, default=0, metavar="C", help="with --clustered: refine a shortlist of C rows on the exact f32 rows")
    a = ap.parse_args()
    if a.refine and not a.clustered:
        ap.error("--refine needs --clustered (the exact f32 index)")
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    n, dim = a.rows, a.dim
    stride = (dim + 15) // 16 * 16
    out = {"rows": n, "dim": dim, "stride": stride, "nlist": a.nlist, "k": a.k, "clustered": a.clustered,
           "shader_clock_mhz_before": clock_mhz(lib)}

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
        cent_np, mn, mx = ivfsq8.train(sample, a.nlist, centroids=coarse)
        out["train"] = {"rows": int(sample.shape[0]), "seconds": time.perf_counter() - t0, "spread": a.spread}
        del sample
    else:
        # the centroids: rows 0, n / nlist, 2 n / nlist, ... of the same fill
        rows = torch.arange(a.nlist, dtype=torch.int64, device="cuda") * (n // a.nlist)
        cent = torch.empty((a.nlist, dim), dtype=torch.float32, device="cuda")
        _lib.check(lib.lb_gpu_fill_uniform_rows_device(0, cent.data_ptr(), rows.data_ptr(), a.nlist, dim, 12345, None))
        torch.cuda.synchronize()
        cent_np = cent.cpu().numpy()
        mn, mx = np.full(dim, -0.5, np.float32), np.full(dim, 0.5, np.float32)

        def draw(cnt, dst, r0=0, seed=12345):
            _lib.check(lib.lb_gpu_fill_uniform_device(0, dst.data_ptr(), cnt * dim, seed, r0 * dim, None))

    h = ivfsq8.IVFSQ8(mn, mx, cent_np)
    h.reserve(n)
    enc = sq8.SQ8Encoder(dim)  # the same vectors under the same bounds: the same codes
    enc.set_bounds(mn, mx)
    enc.reserve(n)
    exact = None
    if a.clustered:  # the f32 rows themselves, for the recall
        exact = gpu.Index(gpu.GPUConfig(DeviceID=0, Dimension=dim))
        exact.reserve(n)
    buf = torch.empty((min(a.piece, n), dim), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    add_s = 0.0
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
        enc.add_vectors_device(cnt, buf.data_ptr())
        if exact is not None:
            exact.add_device(cnt, buf.data_ptr())
    del buf
    sizes = h.list_sizes()
    out["add"] = {"seconds": add_s, "rows_per_s": n / add_s, "pieces": -(-n // a.piece)}
    out["lists"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}
    per_row = stride + 4 * 3  # the codes once; assign and the two lists
    out["hbm_bytes"] = h.hbm_bytes
    out["hbm_bytes_per_row_terms"] = n * per_row
    out["hbm_bytes_beyond_rows"] = h.hbm_bytes - n * per_row  # spare capacity, bounds, offsets, the coarse index
    out["same_codes_as_the_flat_handle"] = bool(np.array_equal(h.codes(0, min(n, 4096)), enc.get_codes(0, min(n, 4096))))

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

    def refined(nq, nprobe, f32_truth):
        """the shortlist search, the refine and both chained: p50s and the refined recall"""
        short = lambda: h.search_device(nq, Q.data_ptr(), a.refine, nprobe, SD.data_ptr(), SL.data_ptr())  # noqa: E731
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
            prof = []
            for _ in range(3):
                run()
                prof.append(h.last_timing())
            h.set_profiling(False)
            steps = [float(np.median([p[i] for p in prof])) for i in range(5)]
            st = h.last_search_stats()
            got = L[:nq].cpu().numpy()
            recall = float(np.mean([np.intersect1d(got[j], truth[j]).size / a.k for j in range(nq)]))
            scan_bytes = st[1] * (stride + 8)
            cell = {"nq": nq, "nprobe": nprobe, "p50_ms": ms, "flat_sq8_p50_ms": flat_ms}
            cell.update(dict(zip(STEPS, steps)))
            cell.update({"rows_scanned": st[1], "max_rows_per_query": st[2], "selected_from_lds": st[3], "scan_bytes": scan_bytes,
                         "scan_gb_per_s": scan_bytes / max(steps[3], 1e-6) / 1e6, "recall_at_k_vs_full_sq8": recall})
            if nprobe >= a.nlist:  # every list probed: the flat SQ8 search's own result, bit for bit
                cell["equals_flat_sq8"] = bool(np.array_equal(got, truth) and np.array_equal(D[:nq].cpu().numpy(), truth_d))
            if exact is not None:
                cell["recall_at_k_vs_exact_f32"] = float(np.mean([np.intersect1d(got[j], f32_truth[j]).size / a.k for j in range(nq)]))
            if a.refine:
                cell["refine"] = refined(nq, nprobe, f32_truth)
            cells.append(cell)
    out["cells"] = cells
    out["shader_clock_mhz_after"] = clock_mhz(lib)
    print(json.dumps(out))
    enc.Close()
    h.Close()
    if exact is not None:
        exact.Close()


if __name__ == "__main__":
    main()
