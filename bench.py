#!/usr/bin/env python3
"""bench.py -- the reference's headline metric on MI355X.

Metric (BASELINE.json): k-NN queries/sec at batch = 1024, k = 100 on 1M x 768 f32 (cosine, brute force),
plus (--full) p50 single-query latency.  One "step" = one batch of 1024 queries searched over the whole job's corpus,
inputs resident in HBM.

  N = 1 (default)      BASELINE config 2: 1M x 768 cosine on one GPU.  With --full, secondary legs on the same line:
                       split-bf16 candidates, p50 latency + scan roofline, batch sweep, PQ/ADC (config 4,
                       100M x m=96), filtered hybrid (config 5, one GPU's share), oracle parity, CPU baseline.
  N > 1, weak          (default) the corpus grows with N: N x 1M rows with ids 0 .. N*1M-1, partitioned by the
                       reference's RingSharder run with 8 ring shards per GPU packed onto the GPUs by size
                       (longbow_amd.sharded.GpuPartition); every rank searches the same 1024 queries over ITS
                       rows, one RCCL all-gather moves the per-shard top-k, every rank merges.  A unit of
                       `value` is one query searched over 1M rows: value = 1024 * N / step_time (per-GPU work
                       fixed up to the ring's residual skew, which is reported, not hidden).
  N > 1, --scaling strong   BASELINE config 3: a FIXED 10M x 768 dot corpus partitioned the same way;
                       value = global queries/s = 1024 / step_time; N = 1 holds all 10M rows.

One rank per GPU.  `python bench.py --gpus N` with no WORLD_SIZE in the environment starts the N ranks itself
(torch.distributed.run as a child process, BEFORE this process imports torch or touches the GPU) and relays rank 0's
JSON line; under `python -m torch.distributed.run ... bench.py --gpus N` it is one of the ranks.  The exchange is the
library's own RCCL path (lb_gpu_comm_*, LB_BENCH_COMM=lib, default; =torch: torch.distributed's all-gather).
Prints ONE JSON line on rank 0.

A plain run does what the headline needs and nothing else: it builds the index, warms up, times the steps and prints
the line (metric, value, ms_per_step, the configuration, and the roofline of the timed steps' own HIP events).  --full
adds everything else to the same line: the chip's clock behind the steps, the other candidate modes, single-query
latency, the batch sweep, concurrent callers, the oracle parity gate, the CPU baseline, the `strong_c3` leg (BASELINE
config 3: a fixed 10M x 768 dot corpus over the N GPUs) and configs 1, 4 and 5.  --no-fast, --no-legs, --no-cpu-baseline
and --cpu-queries trim a --full run; without --full there is nothing for them to trim.

--dump-outputs DIR also writes the headline's last timed step (labels and distances of every query) as DIR/*.npy; the
inputs are generated from fixed seeds, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_ROWS, DIM, BATCH, K = 1_000_000, 768, 1024, 100
METRIC_COSINE, METRIC_DOT = 1, 2
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X dense f32 MFMA (MI355X_MICROARCH.md, chip-level parameters)
PEAK_HBM_GBS = 8000.0          # HBM3E spec
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense bf16 MFMA (same guide)
CAND_F32, CAND_IMAGE, CAND_INREG, CAND_AUTO = 0, 1, 2, 3  # lb_candidate_mode


def host_cores():
    """CPU threads this process may really use: min(affinity, cgroup v2 cpu.max quota)."""
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            cores = max(1, min(cores, int(int(quota) / int(period))))
    except Exception:
        pass
    return cores


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def timed_ms(fn, torch, dev, n=8, skip=2):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append(1e3 * (time.perf_counter() - t0))
    return median(ts[skip:])


def rank_ids(part, rank, global_rows):
    """ascending ids of [0, global_rows) that the partition gives to GPU `rank`"""
    out = []
    step = 4_000_000
    for a in range(0, global_rows, step):
        ids = np.arange(a, min(global_rows, a + step), dtype=np.uint64)
        out.append(ids[part.GetGpus(ids) == rank])
    return np.concatenate(out).astype(np.int64)


# ---------------------------------------------------------------------------------------------------
# secondary legs (--full, N = 1 only)
# ---------------------------------------------------------------------------------------------------
def route_roof_ms(kind, form, B, rows):
    """time the route's contraction needs at the dense MFMA peak of its operand type, and what it is called"""
    flop = 2.0 * B * rows * DIM
    if kind == 4 and form == 0:
        return flop / (PEAK_F32_MFMA_TFLOPS * 1e12) * 1e3, "mfma_f32"
    if form == 3:
        return flop / (PEAK_BF16_MFMA_TFLOPS * 1e12) * 1e3, "mfma_f16_1_product"
    return 3.0 * flop / (PEAK_BF16_MFMA_TFLOPS * 1e12) * 1e3, "mfma_bf16_3_products"


def leg_batch_sweep(torch, dev, idx, Q, rows):
    """HBM-bound regime: whole-search time vs batch size (the reference's live multi-query path issues small
    batches sequentially, internal/store/vector_search_action.go:73)"""
    out = []
    stream = torch.cuda.current_stream(dev).cuda_stream
    for B in (1, 2, 4, 8, 16, 32, 64, 128, 256, 384, 512, 1024):
        od = torch.empty((B, K), device=dev)
        ol = torch.empty((B, K), dtype=torch.int64, device=dev)
        q = Q[:B].contiguous()
        ms = timed_ms(lambda: idx.search_device(B, q.data_ptr(), K, od.data_ptr(), ol.data_ptr(), stream), torch, dev, n=9, skip=3)
        # binding roof of the batch: the corpus stream (HBM) or the contraction of the route the library took (MFMA)
        kind, form, rname = idx.last_route
        hbm_ms = 4.0 * rows * DIM / (PEAK_HBM_GBS * 1e9) * 1e3  # algorithmic: the f32 corpus once
        # what the pass physically reads: the f32 rows, or (fp16 route with the index's fp16 copy) 2 bytes per element
        bpe = 2 if (form == 3 and idx.f16_image_bytes > 0) else 4
        hbm_phys_ms = bpe * rows * DIM / (PEAK_HBM_GBS * 1e9) * 1e3
        mfma_ms, mname = route_roof_ms(kind, form, B, rows) if kind != 0 else (0.0, "")
        out.append({"batch": B, "ms": round(ms, 4), "ms_per_query": round(ms / B, 5), "queries_per_s": round(B / ms * 1e3, 1),
                    "route": rname, "corpus_read_equiv_TBs": round(4.0 * rows * DIM / (ms * 1e-3) / 1e12, 3),
                    # (an f32-corpus EQUIVALENT over 8 TB/s, above 1 when 2-byte elements are read: a speed-up over the
                    # algorithmic stream, NOT a roofline fraction -- that is frac_of_binding_roof, on the bytes physically read)
                    "f32_equivalent_over_8TBs": round(hbm_ms / ms, 4), "corpus_bytes_per_element_read": bpe,
                    "binding_roof": "hbm" if hbm_phys_ms >= mfma_ms else mname,
                    "frac_of_binding_roof": round(max(hbm_phys_ms, mfma_ms) / ms, 4)})
    return out


def leg_pq_adc(torch, dev, lib, _lib, cores, check=True):
    """BASELINE config 4: 100M x 768 -> PQ (m = 96, 8-bit) codes encoded ON THE GPU from synthetic vectors,
    ADC k-NN, k = 100, B = 1."""
    import ctypes as C
    from longbow_amd import pq
    from oracle import oracle_c as oc
    n, dims, M = 100_000_000, 768, 96
    free_b, _ = torch.cuda.mem_get_info(dev)
    if free_b < 24 * 2**30:
        return {"skipped": "needs ~16 GB of free HBM"}
    cb = oc.fill_uniform(M * 256 * (dims // M), 7).reshape(M, 256, dims // M)
    enc = pq.PQEncoder(pq.serialize_codebooks(cb), device=dev.index or 0)
    enc.reserve(n)
    CH = 2_000_000
    buf = torch.empty((CH, dims), device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for r0 in range(0, n, CH):
        _lib.check(lib.lb_gpu_fill_uniform_device(dev.index or 0, buf.data_ptr(), CH * dims, 12345, r0 * dims, None))
        enc.add_vectors_device(CH, buf.data_ptr())
    enc_s = time.perf_counter() - t0
    del buf
    Q = torch.empty((4, dims), device=dev)
    _lib.check(lib.lb_gpu_fill_uniform_device(dev.index or 0, Q.data_ptr(), Q.numel(), 42, 0, None))
    od = torch.empty((4, K), device=dev)
    ol = torch.empty((4, K), dtype=torch.int64, device=dev)
    ms1 = timed_ms(lambda: enc.search_device(1, Q.data_ptr(), K, od.data_ptr(), ol.data_ptr()), torch, dev, n=12, skip=4)
    ms2 = timed_ms(lambda: enc.search_device(2, Q.data_ptr(), K, od.data_ptr(), ol.data_ptr()), torch, dev, n=8, skip=3)
    ms4 = timed_ms(lambda: enc.search_device(4, Q.data_ptr(), K, od.data_ptr(), ol.data_ptr()), torch, dev, n=8, skip=3)
    lab, dist = ol.cpu().numpy().copy(), od.cpu().numpy().copy()
    # the batch results must equal each query's own single-query search (two queries share a pass over the codes)
    pair_ok = True
    for i in range(4):
        enc.search_device(1, Q[i:i + 1].contiguous().data_ptr(), K, od.data_ptr(), ol.data_ptr())
        pair_ok = pair_ok and bool(np.array_equal(ol.cpu().numpy()[0], lab[i]) and np.array_equal(od.cpu().numpy()[0], dist[i]))
    time.sleep(2.0)  # a rested chip: what a single query arriving at an idle server sees (clocks recover in ~1 s)
    rested = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        enc.search_device(1, Q.data_ptr(), K, od.data_ptr(), ol.data_ptr())
        rested.append(1e3 * (time.perf_counter() - t0))
    enc.set_profiling(True)  # HIP events on the search stream around the pass over the codes
    kms, dms = [], []
    for _ in range(8):
        enc.search_device(1, Q.data_ptr(), K, od.data_ptr(), ol.data_ptr())
        a, b = enc.last_timing()
        kms.append(a)
        dms.append(b)
    enc.set_profiling(False)
    k_ms, d_ms = median(kms[2:]), median(dms[2:])
    enc.set_prefilter(False)  # the exact f32-table pass over every row (same results, A/B)
    try:
        ms_exact = timed_ms(lambda: enc.search_device(1, Q.data_ptr(), K, od.data_ptr(), ol.data_ptr()), torch, dev, n=8, skip=3)
        same = bool(np.array_equal(ol.cpu().numpy()[:1], lab[:1]) and np.array_equal(od.cpu().numpy()[:1], dist[:1]))
    finally:
        enc.set_prefilter(True)
    res = {
        "workload": "100M x 768 f32 -> PQ m=96 K=256 codes (9.6 GB), asymmetric distance, k=100, B=1",
        "ms_per_query": round(ms1, 4), "queries_per_s": round(1e3 / ms1, 1),
        "ms_per_query_after_2s_idle": round(min(rested), 4),
        "ms_per_query_at_B2": round(ms2 / 2, 4), "ms_per_query_at_B4": round(ms4 / 4, 4),
        "batch_note": "batches: FOUR queries share one pass over the codes (their byte tables interleaved, one LDS gather per code byte "
                      "for all four; a remainder of two or three runs as a pair + one) -- the pass is bound by the LDS gathers, not by "
                      "the stream; each query's result equals its single-query search",
        "batch_equals_single_query_searches": pair_ok,
        "roofline": {"bound": "hbm", "kernel": "adc_prefilter_kernel", "achieved": round(n * M / (k_ms * 1e-3) / 1e9, 1),
                     "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(n * M / (k_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                     "kernel_ms": round(k_ms, 4), "whole_search_device_ms": round(d_ms, 4),
                     "whole_search_frac_of_8TBs": round(n * M / (ms1 * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                     "whole_search_device_frac_of_8TBs": round(n * M / (d_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                     "algorithmic_bytes_per_query": n * M + 4 * M * 256 + 12 * K},
        "exact_f32_table_pass_ms": round(ms_exact, 4), "prefilter_equals_exact_pass": same,
        "encode": {"vectors": n, "seconds_incl_generation": round(enc_s, 2), "vectors_per_s": round(n / enc_s, 0)},
    }
    if check:  # oracle over ALL codes for one query (threaded restatement of simd.ADCDistanceBatch on the GPU's codes)
        from concurrent.futures import ThreadPoolExecutor
        codes = enc.get_codes()
        table = oc.build_adc_table(cb, Q[0].cpu().numpy())
        step = (n + cores - 1) // cores
        with ThreadPoolExecutor(max_workers=cores) as ex:
            d = np.concatenate(list(ex.map(lambda a: oc.adc_batch(table, codes[a:a + step]), range(0, n, step))))
        oi, odist, _ = oc.topk_canonical(d, K)
        sub = np.random.default_rng(1).integers(0, n, 16)
        enc_ok = all(np.array_equal(codes[r], oc.pq_encode(cb, oc.fill_uniform(dims, 12345, int(r) * dims))) for r in sub)
        res["parity"] = {"query_vs_oracle_ids_equal": bool(np.array_equal(lab[0], oi)),
                         "query_vs_oracle_dist_bit_equal": bool(np.array_equal(dist[0], odist)),
                         "encode_vs_oracle_rows_checked": int(len(sub)), "encode_ok": bool(enc_ok),
                         "ok": bool(np.array_equal(lab[0], oi) and np.array_equal(dist[0], odist) and enc_ok and same and pair_ok)}
        del codes
    enc.Close()
    return res


def leg_config1(torch, dev, lib, _lib, nq=256):
    """BASELINE config 1, the reference's own CPU-runnable case (cmd/bench-tool/main.go:120-210: --dim 128, ingest in
    batches of 1000, then sequential VectorSearch actions of ONE random query, k = 10): 10k x 128 f32, L2.  The reference
    runs it on its CPU path (plumbing, no GPU); here the CPU restatement is timed beside the GPU index at the size where the
    reference's brute-force index actually lives (internal/store/adaptive_index.go:602-615) -- one query per call through the
    host-pointer entry (gpu.Index.Search) and through the device-pointer entry.  Every answer is checked against the oracle."""
    from longbow_amd import gpu
    from oracle import oracle_c as oc
    n, d, k = 10_000, 128, 10
    di = dev.index or 0
    X = oc.fill_uniform(n * d, 12345).reshape(n, d)
    Qh = oc.fill_uniform(nq * d, 42).reshape(nq, d)
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=di, Dimension=d, Metric=0))
    t0 = time.perf_counter()
    for r0 in range(0, n, 1000):  # bench-tool --batch-size=1000
        idx.Add(None, X[r0:r0 + 1000])
    ingest_s = time.perf_counter() - t0
    want_i, want_d = oc.search_batch(0, Qh, X, k, nthreads=host_cores())
    # CPU restatements, sequential single queries on ONE thread as bench-tool issues them
    t0 = time.perf_counter()
    for i in range(nq):
        oc.search_batch(0, Qh[i:i + 1], X, k, nthreads=1)
    scalar_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i in range(nq):
        oc.cpu_baseline(0, Qh[i:i + 1], X, k, nthreads=1, simd=1)
    simd_s = time.perf_counter() - t0
    # GPU: host-pointer entry (borrowed buffers in, results out: what gpu.Index.Search does), one query per call
    od, ol = np.empty((1, k), np.float32), np.empty((1, k), np.int64)
    ok = True
    lat = []
    for rep in range(3):
        for i in range(nq):
            q = np.ascontiguousarray(Qh[i:i + 1])
            t1 = time.perf_counter()
            _lib.check(lib.lb_gpu_index_search(idx._h, 1, q.ctypes.data, k, od.ctypes.data, ol.ctypes.data))
            if rep > 0:
                lat.append(1e3 * (time.perf_counter() - t1))
            ok = ok and bool(np.array_equal(ol[0], want_i[i]) and np.array_equal(od[0], want_d[i]))
    lat.sort()
    # device-pointer entry (inputs and outputs resident in HBM)
    Qd = torch.from_numpy(Qh).to(dev)
    dd = torch.empty((1, k), device=dev)
    dl = torch.empty((1, k), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    dlat = []
    for rep in range(3):
        for i in range(nq):
            q1 = Qd[i:i + 1]
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            idx.search_device(1, q1.data_ptr(), k, dd.data_ptr(), dl.data_ptr(), stream)
            if rep > 0:
                dlat.append(1e3 * (time.perf_counter() - t1))
    dlat.sort()
    route = idx.last_route[2]
    idx.Close()
    pct = lambda xs, p: xs[min(len(xs) - 1, int(len(xs) * p))]
    return {"workload": "10k x 128 f32 L2, k=10, one random query per call, sequential (bench-tool --dim 128 --batch-size 1000)",
            "ingest_10_batches_of_1000_s": round(ingest_s, 4),
            "cpu": {"kind": "port", "cores": 1,
                    "scalar_canonical_queries_per_s": round(nq / scalar_s, 1), "simd_port_queries_per_s": round(nq / simd_s, 1),
                    "bytes_per_query": 4 * n * d},
            "gpu_host_pointer_entry": {"p50_ms": round(pct(lat, 0.5), 4), "p99_ms": round(pct(lat, 0.99), 4),
                                       "queries_per_s": round(1e3 * len(lat) / sum(lat), 1)},
            "gpu_device_pointer_entry": {"p50_ms": round(pct(dlat, 0.5), 4), "p99_ms": round(pct(dlat, 0.99), 4)},
            "route": route,
            "note": "a fixed cost, not a stream: 5 MB of corpus is 0.6 us of HBM; the time is launches + one host wake-up",
            "parity": {"checked_queries": nq, "vs": "oracle, bit-equal lists", "ok": ok}}


def leg_concurrent_callers(lib, idx, Q, threads=8, secs=1.0):
    """gpu.Index.Search as the reference calls it (internal/gpu/faiss_gpu.go:108-145): ONE query per call through the
    host-pointer entry, from `threads` concurrent callers (goroutines there, host threads here; ctypes releases the GIL).
    With request combining (the library default) overlapping calls are answered by one batched device search; without it every
    call streams the corpus for itself."""
    import threading
    Qh = Q[:threads].cpu().numpy()
    out = {}
    for name, comb in (("combined", 1), ("each_call_on_its_own", 0)):
        idx.set_search_combining(comb)
        before = idx.combining_stats
        barrier = threading.Barrier(threads)
        res = {}

        def worker(t):
            q = np.ascontiguousarray(Qh[t])
            od, ol = np.empty(K, np.float32), np.empty(K, np.int64)
            for _ in range(3):
                lib.lb_gpu_index_search(idx._h, 1, q.ctypes.data, K, od.ctypes.data, ol.ctypes.data)
            barrier.wait()
            t0 = time.perf_counter()
            lat = []
            while time.perf_counter() - t0 < secs:
                a = time.perf_counter()
                lib.lb_gpu_index_search(idx._h, 1, q.ctypes.data, K, od.ctypes.data, ol.ctypes.data)
                lat.append(time.perf_counter() - a)
            res[t] = (lat, time.perf_counter() - t0)

        ths = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        lat = sorted(x for l, _ in res.values() for x in l)
        after = idx.combining_stats
        out[name] = {"queries_per_s": round(sum(len(l) / dt for l, dt in res.values()), 1),
                     "p50_ms": round(1e3 * lat[len(lat) // 2], 4), "p99_ms": round(1e3 * lat[int(len(lat) * 0.99)], 4),
                     "combined_batches": after[0] - before[0], "requests_in_them": after[1] - before[1]}
    idx.set_search_combining(1)
    out["threads"] = threads
    out["entry"] = "lb_gpu_index_search (host pointers, 1 query per call)"
    return out


def leg_filtered_hybrid(torch, dev, lib, _lib, cores):
    """BASELINE config 5 on ONE GPU's share: 1.25M x 1536 f32 dot, int64 metadata `< 10` (10 % of the rows),
    batch 256, dense side asks for 2k = 200 (internal/store/hybrid_search.go:62), RRF k = 60 with a synthetic
    sparse ranking (BM25 stays on the CPU in the reference)."""
    from concurrent.futures import ThreadPoolExecutor
    from longbow_amd import gpu
    from oracle import oracle_c as oc
    rows, D5, B5 = 1_250_000, 1536, 256
    di = dev.index or 0
    X = torch.empty((rows, D5), device=dev)
    Q = torch.empty((B5, D5), device=dev)
    _lib.check(lib.lb_gpu_fill_uniform_device(di, X.data_ptr(), X.numel(), 12345, 0, None))
    _lib.check(lib.lb_gpu_fill_uniform_device(di, Q.data_ptr(), Q.numel(), 42, 0, None))
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=di, Dimension=D5, Metric=METRIC_DOT))
    idx.add_device(rows, X.data_ptr())
    meta = np.random.default_rng(5).integers(0, 100, rows).astype(np.int64)
    visible = np.flatnonzero(meta < 10)
    # synthetic sparse ranking: 2k distinct visible ids per query (ids are unique within a ranked list)
    rs6 = np.random.default_rng(6)
    sparse = torch.from_numpy(np.stack([visible[rs6.choice(len(visible), 2 * K, replace=False)] for _ in range(B5)])).to(dev)
    dd = torch.empty((B5, 2 * K), device=dev)
    dl = torch.empty((B5, 2 * K), dtype=torch.int64, device=dev)
    oi = torch.empty((B5, K), dtype=torch.int64, device=dev)
    osc = torch.empty((B5, K), device=dev)
    t_filter = timed_ms(lambda: idx.filter_column(meta, "<", 10), torch, dev)
    t_dense = timed_ms(lambda: idx.search_device(B5, Q.data_ptr(), 2 * K, dd.data_ptr(), dl.data_ptr()), torch, dev)
    t_fuse = timed_ms(lambda: _lib.check(lib.lb_gpu_rrf_fuse_device(di, B5, 2 * K, dl.data_ptr(), 2 * K, sparse.data_ptr(), 60, K,
                                                                     oi.data_ptr(), osc.data_ptr(), None)), torch, dev)
    lab, dist = dl.cpu().numpy(), dd.cpu().numpy()
    idx_route = idx.last_route[2]
    Xv = X[torch.from_numpy(visible).to(dev)].cpu().numpy()  # the oracle only needs the visible rows
    Qh = Q.cpu().numpy()
    ok = bool(np.all(meta[lab] < 10))
    checked = (0, 37, 74, 111, 148, 185, 222, B5 - 1)
    for qi in checked:
        step = (len(visible) + cores - 1) // cores
        with ThreadPoolExecutor(max_workers=cores) as ex:
            d = np.concatenate(list(ex.map(lambda a: oc.batch_flat(METRIC_DOT, Qh[qi], Xv[a:a + step]), range(0, len(visible), step))))
        ti, td, _ = oc.topk_canonical(d, 2 * K)
        ok = ok and bool(np.array_equal(lab[qi], visible[ti]) and np.array_equal(dist[qi], td))
        ri, rs = oc.rrf(lab[qi], sparse[qi].cpu().numpy(), 60, K)
        ok = ok and bool(np.array_equal(oi[qi].cpu().numpy(), ri) and np.array_equal(osc[qi].cpu().numpy(), rs))
    idx.Close()
    per = t_dense + t_fuse
    return {"workload": "1.25M x 1536 f32 dot (one GPU's share of 10M), int64 predicate < 10 (10 % visible), batch 256, dense 2k=200, RRF k=60",
            "predicate_to_mask_ms": round(t_filter, 4), "dense_filtered_search_ms": round(t_dense, 4), "rrf_fusion_ms": round(t_fuse, 4),
            "ms_per_batch": round(per, 4), "queries_per_s": round(B5 / per * 1e3, 1),
            "visible_rows_read_equiv_TBs": round(4.0 * len(visible) * D5 / (t_dense * 1e-3) / 1e12, 3),
            "visible_rows_frac_of_8TBs": round(4.0 * len(visible) * D5 / (t_dense * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
            "route": idx_route,
            "parity": {"checked_queries": len(checked), "ok": ok}}


def launch_ranks(args, argv):
    """--gpus N > 1 without a launcher: start N fresh rank processes (torch.distributed.run) as a CHILD of this
    process, relay rank 0's JSON line, exit with the child's code.  Nothing in this process has imported torch or
    touched the GPU (a process that has initialised HIP must never exec or be re-used as a launcher on this pool)."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["LB_BENCH_CHILD"] = "1"
    if os.environ.get("LB_BENCH_LAUNCH_ECHO") == "1":  # CPU test hook: show what would be started, and from what state
        print(json.dumps({"cmd": cmd, "torch_imported": "torch" in sys.modules,
                          "longbow_imported": any(m.startswith("longbow_amd") for m in sys.modules)}), flush=True)
        return 0
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for out in proc.stdout:
        out = out.rstrip("\n")
        if out.startswith("{") and '"metric"' in out:
            line = out
        else:
            print(out, file=sys.stderr, flush=True)
    rc = proc.wait()
    if line is not None:
        print(line, flush=True)
    return rc if rc != 0 else (0 if line is not None else 1)


class Job:
    """what every leg needs: torch, device, library, rank / world, the process group switch"""


def build_index(job, metric, rows_global, part, mode):
    """this rank's shard of a synthetic corpus of rows_global rows (ids 0 .. rows_global-1, content a function of the
    id), generated in HBM: SURVEY 8d -- uniform [0,1), corpus seed 12345"""
    torch, dev, lib, _lib, gpu = job.torch, job.dev, job.lib, job._lib, job.gpu
    di = job.local_rank
    my_ids = rank_ids(part, job.rank, rows_global) if job.use_dist else None
    rows = int(my_ids.size) if my_ids is not None else rows_global
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=di, Dimension=DIM, Metric=metric))
    idx.set_candidate_mode(mode)
    idx.reserve(rows)
    X = None
    CH = 1_000_000
    if my_ids is None:
        if rows <= 2 * CH:
            X = torch.empty((rows, DIM), device=dev)
            _lib.check(lib.lb_gpu_fill_uniform_device(di, X.data_ptr(), X.numel(), 12345, 0, None))
            idx.add_device(rows, X.data_ptr())
        else:
            buf = torch.empty((CH, DIM), device=dev)
            for r0 in range(0, rows, CH):
                c = min(CH, rows - r0)
                _lib.check(lib.lb_gpu_fill_uniform_device(di, buf.data_ptr(), c * DIM, 12345, r0 * DIM, None))
                idx.add_device(c, buf.data_ptr())
            del buf
    else:
        buf = torch.empty((min(CH, max(rows, 1)), DIM), device=dev)
        ids_t = torch.from_numpy(my_ids).to(dev)
        for r0 in range(0, rows, CH):
            c = min(CH, rows - r0)
            _lib.check(lib.lb_gpu_fill_uniform_rows_device(di, buf.data_ptr(), ids_t[r0:r0 + c].data_ptr(), c, DIM, 12345, None))
            idx.add_device(c, buf.data_ptr(), ids_t[r0:r0 + c].data_ptr())
        del buf
    return idx, X, rows


def make_searcher(job, idx):
    """the cross-shard step: lb_gpu_comm (RCCL inside liblongbow_gpu.so) by default, torch.distributed on request;
    a communicator that cannot be stood up on EVERY rank falls back to torch on all of them (and says so)"""
    if not job.use_dist:
        return None, "single shard"
    from longbow_amd.sharded import CommSearcher, ShardedSearcher
    torch, dist = job.torch, job.dist
    kind = os.environ.get("LB_BENCH_COMM", "lib")
    if kind == "lib":
        searcher, err = None, ""
        try:
            searcher = CommSearcher(idx, job.rank, job.world, device_index=job.local_rank, transport="rccl")
            searcher.prepare(BATCH, K)  # exchange buffers sized now: a failure is agreed on below, before any collective
        except Exception as e:  # noqa: BLE001 -- reported below
            err = f"{type(e).__name__}: {e}"
        ok = torch.tensor([1 if searcher is not None else 0], device=job.dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            return searcher, "lb_gpu_comm (RCCL all-gather inside liblongbow_gpu.so) + device merge"
        if searcher is not None:
            searcher.close()
        kind = f"torch (lb_gpu_comm could not be initialised on every rank: {err or 'a peer failed'})"
    return (ShardedSearcher(idx, job.rank, job.world, device=job.dev, force_collective=True),
            f"{kind if kind != 'torch' else 'torch.distributed'} all-gather + device merge")


def timed_steps(job, idx, searcher, Q, steps, warmup):
    """W untimed + K timed steps bracketed by barrier + synchronize; MAX over ranks; library event timing per class"""
    torch, dist, dev = job.torch, job.dist, job.dev
    B = Q.shape[0]
    out_d = torch.empty((B, K), device=dev)
    out_l = torch.empty((B, K), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def step():
        if searcher is not None:
            return searcher.search(Q, K)
        idx.search_device(B, Q.data_ptr(), K, out_d.data_ptr(), out_l.data_ptr(), stream)
        return out_l, out_d

    def barrier():
        if job.use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(warmup):
        step()
    idx.set_profiling(True)  # HIP events on the search stream around each kernel class
    cls_ms = {"gemm": 0.0, "select": 0.0, "rerank": 0.0, "scan": 0.0, "total": 0.0}
    gemm_launches, fallbacks = 0, 0
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        lab, dd = step()
        tm = idx.last_timing()
        gemm_launches += tm["gemm"][1]
        for c in cls_ms:
            cls_ms[c] += tm[c][0]
        fallbacks += idx.last_fallbacks
    barrier()
    elapsed = time.perf_counter() - t0
    idx.set_profiling(False)
    if job.use_dist:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # labels / dist: what the LAST timed step returned (the buffers are not touched again before this copy)
    return {"elapsed": elapsed, "cls_ms": cls_ms, "gemm_launches": gemm_launches, "fallbacks": fallbacks,
            "labels": lab.cpu().numpy().copy(), "dist": dd.cpu().numpy().copy(), "step": step}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each [B, ...] array as out_dir/<name>.npy, float32 stays float32 and everything else becomes float64
    (labels: ids < 2^53, exact).  Past DUMP_MAX_BYTES in all, the same fixed, seeded sample of rows is taken from every
    array and its row numbers are written as query_rows.npy."""
    out = {n: np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64) for n, a in arrays.items()}
    nrows = next(iter(out.values())).shape[0]
    row_bytes = sum(a.nbytes // max(1, a.shape[0]) for a in out.values())
    if row_bytes * nrows > DUMP_MAX_BYTES:
        keep = DUMP_MAX_BYTES // (row_bytes + 8)  # (+ its query_rows entry)
        sel = np.sort(np.random.default_rng(0).choice(nrows, size=keep, replace=False))
        out = {n: a[sel] for n, a in out.items()}
        out["query_rows"] = sel.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for n, a in out.items():
        np.save(os.path.join(out_dir, n + ".npy"), a)


def gather_rows(job, rows):
    if not job.use_dist:
        return [rows]
    torch, dist = job.torch, job.dist
    cnt = torch.tensor([rows], device=job.dev, dtype=torch.int64)
    allc = [torch.zeros_like(cnt) for _ in range(job.world)]
    dist.all_gather(allc, cnt)
    return [int(c.item()) for c in allc]


def shard_report(shard_rows):
    return {"per_rank": shard_rows, "max": max(shard_rows), "mean": round(sum(shard_rows) / len(shard_rows), 1),
            "max_over_mean": round(max(shard_rows) * len(shard_rows) / max(sum(shard_rows), 1), 4)}


def leg_strong_c3(job, part, Q, steps, warmup, global_rows=10_000_000):
    """BASELINE config 3: a FIXED 10M x 768 dot-product corpus over the job's GPUs (N = 1 holds all of it), library
    default candidate mode, per-shard top-k exchanged and merged; value = global queries/s"""
    idx, _, rows = build_index(job, METRIC_DOT, global_rows, part, CAND_AUTO)
    searcher, how = make_searcher(job, idx)
    r = timed_steps(job, idx, searcher, Q, steps, warmup)
    shard_rows = gather_rows(job, rows)
    B = Q.shape[0]
    out = {"workload": "10Mx768 float32 dot-product, corpus sharded across the GPUs, RCCL top-k merge",
           "scaling": "strong", "value": round(B * steps / r["elapsed"], 1), "unit": "queries/s (global, fixed 10M-row corpus)",
           "ms_per_step": round(1e3 * r["elapsed"] / steps, 4), "steps": steps, "candidate_mode": "auto",
           "fallback_queries": int(r["fallbacks"]), "shard_rows": shard_report(shard_rows), "exchange": how,
           "device_ms_per_step": {c: round(v / steps, 4) for c, v in r["cls_ms"].items()}}
    if hasattr(searcher, "close"):
        searcher.close()
    idx.Close()
    job.torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=N_ROWS, help="rows per GPU (weak) / global rows (strong: default 10M)")
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline, run every other measurement and check (clock probe, candidate modes, latency, "
                         "sweep, concurrent callers, oracle parity, CPU baseline, strong C3, configs 1, 4 and 5)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-fast", action="store_true", help="with --full: skip the candidate-mode legs (auto path, split-bf16 image)")
    ap.add_argument("--no-legs", action="store_true",
                    help="with --full: skip the secondary legs (sweep, strong C3, PQ, filtered hybrid)")
    ap.add_argument("--cpu-queries", type=int, default=0, help="with --full: CPU baseline sample size (0 = 16 per core)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (labels, distances) to DIR/<name>.npy, for output-for-output "
                         "comparison of two builds on the same seeded inputs")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and os.environ.get("LB_BENCH_CHILD") != "1":
        sys.exit(launch_ranks(args, sys.argv[1:]))  # before torch / the GPU library are imported

    import torch
    import torch.distributed as dist
    from longbow_amd import _lib, gpu
    from longbow_amd.sharded import GpuPartition

    job = Job()
    job.torch, job.dist, job._lib, job.gpu = torch, dist, _lib, gpu
    job.world = world = int(os.environ.get("WORLD_SIZE", "1"))
    job.rank = rank = int(os.environ.get("RANK", "0"))
    job.local_rank = local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and not (world == 1 and args.gpus == 1):
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}, "
                         "or with no launcher at all (bench.py then starts the ranks itself)")
    torch.cuda.set_device(local_rank)
    job.dev = dev = torch.device("cuda", local_rank)
    # LB_BENCH_FORCE_DIST=1 exercises the collective path (process group, all-gather, merge) even with one
    # rank, so the multi-GPU code can be rehearsed on a single-GPU box.
    job.use_dist = use_dist = world > 1 or os.environ.get("LB_BENCH_FORCE_DIST") == "1"
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    job.lib = lib = _lib.require_gpu(local_rank)
    strong = args.scaling == "strong"
    metric = METRIC_DOT if strong else METRIC_COSINE
    B = args.batch
    global_rows = (10_000_000 if args.rows == N_ROWS else args.rows) if strong else args.rows * world

    # ---- synthetic inputs, generated in HBM (uniform [0,1), corpus seed 12345, queries 42) ----
    shards_per_gpu = 8
    part = GpuPartition(world, shards_per_gpu, 40)
    Q = torch.empty((B, DIM), device=dev)
    _lib.check(lib.lb_gpu_fill_uniform_device(local_rank, Q.data_ptr(), Q.numel(), 42, 0, None))
    # the headline is measured in the STRICT mode (f32 MFMA candidates beyond 384 queries: dtype f32 end to end);
    # the library's default (AUTO: split-bf16 candidates, same results) is the auto_path leg below
    idx, X, rows = build_index(job, metric, global_rows, part, CAND_F32)
    searcher, how = make_searcher(job, idx)
    r = timed_steps(job, idx, searcher, Q, args.steps, args.warmup)
    elapsed, cls_ms, step = r["elapsed"], r["cls_ms"], r["step"]
    gemm_ms, gemm_launches, fallbacks = cls_ms["gemm"], r["gemm_launches"], r["fallbacks"]
    lab_h, dist_h = r["labels"], r["dist"]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"labels": lab_h, "distances": dist_h})
    shard_rows = gather_rows(job, rows)
    stream = torch.cuda.current_stream(dev).cuda_stream

    ms_per_step = 1e3 * elapsed / args.steps
    if strong:
        value = B * args.steps / elapsed                     # global queries/s over the fixed corpus
        metric_name = "k-NN queries/sec (batch=1024, k=100), 10Mx768 f32 dot, corpus sharded over the GPUs"
        workload = "10Mx768 float32 dot-product, corpus sharded across the GPUs, RCCL top-k merge"
    else:
        value = B * (global_rows / float(N_ROWS)) * args.steps / elapsed  # unit: one query over 1M rows
        metric_name = "k-NN queries/sec (batch=1024, k=100), 1Mx768 f32"
        workload = "1Mx768 float32 cosine, batch=1024 queries, k=100, brute-force"

    flops_per_step = 2.0 * B * rows * DIM
    bytes_per_step = 4.0 * rows * DIM + 4.0 * B * DIM + 12.0 * B * K
    result = {
        "metric": metric_name, "value": round(value, 1),
        "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": args.scaling, "full": args.full,
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": workload, "dim": DIM, "batch": B, "k": K, "metric": "dot" if strong else "cosine",
                   "global_rows": global_rows, "candidate_mode": "LB_CAND_F32_MFMA (strict; the library default is AUTO: auto_path leg)",
                   "shard_rows": shard_report(shard_rows),
                   "sharding": (f"RingSharder({world * shards_per_gpu}, 40): {shards_per_gpu} ring shards per GPU packed by size "
                                f"(one ring shard per GPU would be {GpuPartition(world, 1, 40).skew():.2f}x skewed) + {how}")
                   if use_dist else "single shard",
                   "unit_of_value": "global queries/s" if strong else "one query searched over 1M x 768 rows"},
        "fallback_queries": int(fallbacks),
        "device_ms_per_step": {c: round(v / args.steps, 4) for c, v in cls_ms.items()},
    }

    if gemm_ms > 0:
        achieved = flops_per_step * args.steps / (gemm_ms * 1e-3) / 1e12
        result["roofline"] = {
            "bound": "mfma", "kernel": "gemm_filter_kernel", "achieved": round(achieved, 2),
            "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_F32_MFMA_TFLOPS, 4),
            # HBM bytes per launch come from PMC counters, which a run cannot collect on itself: null here; the round's own
            # counter passes of this command are in profiles/ (see profiles/README.md)
            "traffic": None,
            "launches_per_step": gemm_launches / args.steps,
            "kernel_ms_per_step": round(gemm_ms / args.steps, 4),
            "flops_per_step": flops_per_step,
            "hbm_algorithmic_bytes_per_step": bytes_per_step,
            "hbm_frac_of_8TBs_at_step_rate": round(bytes_per_step / (ms_per_step * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
        }
    # ---- everything below this line is --full: a plain run has its line and goes straight to the print ----------
    # the chip's clock state right behind the timed steps (the same search runs 1.67-1.95 ms by clock state on one box)
    if args.full:
        try:
            mhz = float(lib.lb_gpu_shader_clock_mhz(local_rank, 2000))
            result["shader_clock_mhz_after_steps"] = round(mhz, 1) if mhz > 0 else None
        except Exception:
            result["shader_clock_mhz_after_steps"] = None

    single = args.full and world == 1 and not use_dist and not strong and X is not None

    def mode_leg(mode, note):
        """the same batch in another candidate mode: identical results required, own roofline"""
        idx.set_candidate_mode(mode)
        for _ in range(2):
            step()
        idx.set_profiling(True)
        f_ms, f_launch, f_fb = 0.0, 0, 0
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
            tm = idx.last_timing()
            f_ms += tm["gemm"][0]
            f_launch += tm["gemm"][1]
            f_fb += idx.last_fallbacks
        torch.cuda.synchronize(dev)
        f_el = time.perf_counter() - t1
        idx.set_profiling(False)
        labf, ddf = step()
        labf, ddf = labf.cpu().numpy(), ddf.cpu().numpy()
        same = bool(np.array_equal(labf, lab_h) and np.array_equal(ddf, dist_h))
        kind, form, rname = idx.last_route
        passes = 1.0 if form == 3 else 3.0
        ach = passes * flops_per_step * args.steps / (f_ms * 1e-3) / 1e12 if f_ms > 0 else 0.0
        kms = f_ms / args.steps
        # bytes the kernel stages from L2 into LDS per step: (corpus rows + query rows) x row bytes, per workgroup tile
        tiles_q = -(-B // 256) if kind in (5, 6) else -(-B // 128)
        row_tiles = -(-rows // 256)
        img_bytes = idx.f16_image_bytes if form == 3 else 0  # the fp16 route's own copy of the corpus (2 B per element)
        stage_bytes = row_tiles * tiles_q * DIM * ((256 * (2 if img_bytes else 4)) + (256 if kind in (5, 6) else 128) * (2 if form == 3 else 4))
        return {"value": round(B * args.steps / f_el, 1), "unit": "queries/s", "ms_per_step": round(1e3 * f_el / args.steps, 4),
                "route": rname, "results_identical_to_f32_mode": same, "fallback_queries": int(f_fb),
                "roofline": {"bound": "mfma", "kernel": rname, "achieved": round(ach, 1),
                             "peak": PEAK_BF16_MFMA_TFLOPS,
                             "unit": f"TFLOP/s ({'fp16, 1 MFMA product' if form == 3 else 'bf16, 3 MFMA products'} per element counted)",
                             "frac": round(ach / PEAK_BF16_MFMA_TFLOPS, 4), "kernel_ms_per_step": round(kms, 4),
                             "launches_per_step": f_launch / args.steps,
                             "l2_to_lds_staged_TBs": round(stage_bytes / (kms * 1e-3) / 1e12, 2) if kms > 0 else None,
                             "hbm_floor_ms": round(4.0 * rows * DIM / (PEAK_HBM_GBS * 1e9) * 1e3, 4),
                             "corpus_bytes_read_per_pass": int((2 if img_bytes else 4) * rows * DIM)},
                "extra_hbm_bytes": int(img_bytes), "note": note}, labf, ddf

    auto_lab = auto_dist = None
    if not args.no_fast and single:
        # ---- the library's DEFAULT path (LB_CAND_AUTO): same exact results, no second copy of the corpus -------
        try:
            result["auto_path"], auto_lab, auto_dist = mode_leg(
                CAND_AUTO,
                "LB_CAND_AUTO, the library default: the cheapest exact route -- here ONE fp16 MFMA product per element over the "
                "index's fp16 copy of the corpus (kept while memory allows: extra_hbm_bytes; error bound 1.1e-3 |q||x|: the finish launch "
                "re-ranks the rows within that bound of the k-th key, a few hundred per query); reported distances/ids come from the "
                "exact f32 re-rank, as in every mode")
            idx.set_f16_image(0)
            result["auto_path_without_fp16_copy"], _, _ = mode_leg(
                CAND_AUTO, "the same with lb_gpu_index_set_f16_image(h, 0): no second copy, the f32 rows are rounded to fp16 in registers "
                           "(what AUTO does when memory is short)")
            idx.set_f16_image(1)
            result["split_bf16_in_registers"], _, _ = mode_leg(
                CAND_INREG, "lb_gpu_index_set_candidate_mode(LB_CAND_SPLIT_BF16_INREG): hi*hi + hi*lo + lo*hi on the bf16 MFMA, both "
                            "f32 operands split in registers (what AUTO falls back to when the corpus norms rule fp16 out)")
        except Exception as e:  # keep the primary line even if an optional leg fails
            result["auto_path"] = {"error": str(e)}
        # ---- opt-in: pre-split bf16 image of the corpus (a second N*D*4-byte copy) --------------------------------
        try:
            result["split_bf16_candidates"], _, _ = mode_leg(
                CAND_IMAGE, "opt-in lb_gpu_index_set_candidate_mode(LB_CAND_SPLIT_BF16): the split contraction over a pre-split image")
            result["split_bf16_candidates"]["extra_hbm_bytes"] = int(4 * rows * DIM)
            result["split_bf16_candidates"]["roofline"]["corpus_bytes_read_per_pass"] = int(4 * rows * DIM)
        except Exception as e:
            result["split_bf16_candidates"] = {"error": str(e)}
        finally:
            try:
                idx.set_candidate_mode(CAND_AUTO)
            except Exception:
                pass

    if single:
        idx.set_candidate_mode(CAND_AUTO)
        # ---- p50 single-query latency (the DoExchange path is single-query) ------------------------
        d1 = torch.empty((1, K), device=dev)
        l1 = torch.empty((1, K), dtype=torch.int64, device=dev)

        def single_query_latency(n_lat=224):
            """(p50, p99 wall clock, p50 of the corpus pass by HIP events, route) of 1-query searches"""
            lat = []
            for i in range(n_lat):  # wall-clock latency, library profiling off
                q1 = Q[i % B:i % B + 1].contiguous()
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                idx.search_device(1, q1.data_ptr(), K, d1.data_ptr(), l1.data_ptr(), stream)
                lat.append(1e3 * (time.perf_counter() - t1))
            route = idx.last_route
            cls = "scan" if route[0] == 0 else "gemm"
            idx.set_profiling(True)  # second pass: HIP events around the corpus pass itself
            pass_ms = []
            for i in range(24):
                q1 = Q[i:i + 1].contiguous()
                idx.search_device(1, q1.data_ptr(), K, d1.data_ptr(), l1.data_ptr(), stream)
                pass_ms.append(idx.last_timing()[cls][0])
            idx.set_profiling(False)
            lat = sorted(lat[24:])
            return lat[len(lat) // 2], lat[min(len(lat) - 1, int(len(lat) * 0.99))], median(pass_ms[4:]), route

        # the library default: with the index's fp16 copy a single query's candidate pass streams 2 bytes per element.
        # Measured twice: straight behind the batch legs above (seconds of MFMA work at the socket's power cap: the HBM-bound
        # pass of a single query then runs ~4 % slower for a while), and again after two idle seconds -- the state a
        # latency-serving index is in, and the one `batch_sweep` below runs in.  Both are reported; the headline p50 is the rested one.
        p50_hot, p99_hot, _, _ = single_query_latency(124)
        time.sleep(2.0)
        p50, p99, pass_p50, route = single_query_latency()
        bpe = 2 if (route[0] == 7 and idx.f16_image_bytes > 0) else 4
        result["p50_latency_ms"] = round(p50, 4)
        result["p99_latency_ms"] = round(p99, 4)
        result["latency_right_behind_the_batch_legs"] = {"p50_latency_ms": round(p50_hot, 4), "p99_latency_ms": round(p99_hot, 4),
                                                         "note": "no idle time after ~20 batched steps per candidate mode; p50_latency_ms is taken after 2 s of idle"}
        result["latency_roofline"] = {
            "bound": "hbm", "kernel": "scan_kernel" if route[0] == 0 else route[2],
            "bytes_per_element_read": bpe,
            "achieved": round(bpe * rows * DIM / (pass_p50 * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": round(bpe * rows * DIM / (pass_p50 * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
            "pass_ms": round(pass_p50, 4),
            "whole_search_frac_of_8TBs_physical": round(bpe * rows * DIM / (p50 * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
            "whole_search_f32_corpus_equivalent_TBs": round(4.0 * rows * DIM / (p50 * 1e-3) / 1e12, 3)}
        if bpe == 2:  # and without the copy: the exact scan over the f32 rows (what rounds 1-2 reported here)
            idx.set_f16_image(0)
            p50s, p99s, scan_p50, _ = single_query_latency(72)
            idx.set_f16_image(1)
            result["latency_without_fp16_copy"] = {
                "p50_latency_ms": round(p50s, 4), "p99_latency_ms": round(p99s, 4), "kernel": "scan_kernel", "scan_kernels_ms": round(scan_p50, 4),
                "achieved": round(4.0 * rows * DIM / (scan_p50 * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": round(4.0 * rows * DIM / (scan_p50 * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                "whole_search_frac_of_8TBs": round(4.0 * rows * DIM / (p50s * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
        if not args.no_legs:
            try:
                result["batch_sweep"] = leg_batch_sweep(torch, dev, idx, Q, rows)  # library default (AUTO)
            except Exception as e:
                result["batch_sweep"] = {"error": str(e)}
            try:
                result["concurrent_single_query_callers"] = leg_concurrent_callers(lib, idx, Q)
            except Exception as e:
                result["concurrent_single_query_callers"] = {"error": str(e)}

        # ---- parity gate + CPU baseline (oracle = test/bench infrastructure, never the product) -----
        from oracle import oracle_c as oc
        Xh = X.cpu().numpy()
        Qh = Q.cpu().numpy()
        cores = host_cores()
        sub = np.arange(0, B, max(1, B // 64))[:64]
        oi, od = oc.search_batch(METRIC_COSINE, Qh[sub], Xh, K, nthreads=cores)
        ok = bool(np.array_equal(oi, lab_h[sub]) and np.array_equal(od, dist_h[sub]))
        result["parity"] = {"checked_queries": int(len(sub)), "index_sets_equal": bool(np.array_equal(oi, lab_h[sub])),
                            "distances_bit_equal": bool(np.array_equal(od, dist_h[sub])), "ok": ok}
        if auto_lab is not None and isinstance(result.get("auto_path"), dict):
            a_ok = bool(np.array_equal(oi, auto_lab[sub]) and np.array_equal(od, auto_dist[sub]))
            result["auto_path"]["parity"] = {"checked_queries": int(len(sub)), "vs": "oracle (full corpus)", "ok": a_ok}
        if not args.no_cpu_baseline:
            nqc = args.cpu_queries or 16 * cores  # 16 full-corpus scans per thread: tens of core-seconds
            nqc = min(nqc, B)
            secs, bi, bd = oc.cpu_baseline(METRIC_COSINE, Qh[:nqc], Xh, K, nthreads=cores, simd=1)
            # the SIMD port sums in 16-lane blocks, so near-ties may swap places or sides of rank k: compare SETS per query
            same_sets = float(np.mean([len(np.intersect1d(bi[i], lab_h[i])) / float(K) for i in range(nqc)]))
            agree = float((bi == lab_h[:nqc]).mean())
            result["cpu_baseline"] = {
                "value": round(nqc / secs, 2), "unit": "queries/s", "cores": cores, "kind": "port",
                "sample": f"{nqc} of the {B} queries, each scanned over the full {rows}x{DIM} corpus "
                          f"(reference idiom: queries partitioned over {cores} threads, SIMD C port of internal/simd)",
                "seconds": round(secs, 2), "index_set_agreement_with_gpu": round(same_sets, 5),
                "label_position_agreement_with_gpu": round(agree, 5),
                "note": "the port is the timed baseline, not the parity oracle (that is `parity`: bit-equal lists); its 16-lane "
                        "summation order moves a few near-ties"}
        del Xh

    # ---- BASELINE config 3 beside the headline, at every N (the fixed-corpus scaling of the same job) ----------
    if hasattr(searcher, "close"):
        searcher.close()
    searcher = None
    if args.full and not args.no_legs and not strong:
        idx.Close()
        idx = None
        X = None
        torch.cuda.empty_cache()
        try:
            result["strong_c3"] = leg_strong_c3(job, part, Q, max(3, args.steps // 4), 1)
        except Exception as e:
            if use_dist:
                raise  # (a rank that skipped a collective leg would strand its peers)
            result["strong_c3"] = {"error": f"{type(e).__name__}: {e}"}

    if single and not args.no_legs:
        # ---- configs 4 and 5 (own corpora; the 1M x 768 index was released above) ----------------------
        cores = host_cores()
        for name, fn in (("config1_10k_x_128", lambda: leg_config1(torch, dev, lib, _lib)),
                         ("pq_adc", lambda: leg_pq_adc(torch, dev, lib, _lib, cores)),
                         ("filtered_hybrid", lambda: leg_filtered_hybrid(torch, dev, lib, _lib, cores))):
            try:
                result[name] = fn()
            except Exception as e:
                result[name] = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.empty_cache()

    if rank == 0:
        print(json.dumps(result), flush=True)
    if idx is not None:
        idx.Close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
