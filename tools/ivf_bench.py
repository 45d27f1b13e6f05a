"""IVF-Flat index (exact k-NN over the probed lists) against the brute-force f32 index on the same rows: one JSON line.

    python tools/ivf_bench.py [--rows 1000000] [--dim 768] [--nlist 256] [--k 100] [--dtype {f32,f16,both,int8}] [--profile-reps 1]

Rows and queries come from the seeded device fill (uniform in [-0.5, 0.5)); the centroids are nlist of the rows (ivf.train with
max_iter = 0 returns its init rows).  Per cell (nprobe x nq): the p50 of the whole search through the device-pointer entry point
as the median of three wall-clock runs after a warm-up (the call returns when the results are on the device); the HIP-event time
of each step (probes, plan, list scan, selection) as the median over --profile-reps further, profiled, runs; rows and bytes
scanned (rows * dim * the element's bytes); the scan pass's bytes per second and its share of 8 TB/s; recall@k against
lb_gpu_index_search on an f32 index with the same rows; and that index's own p50 for the same nq, in the same run.  Also: the add
rate in rows/s, and one ivf.train(nlist = 256, max_iter = 1) on 100k rows with its E-step time.  The shader clock is read before
and after.  A run that finds no GPU fails.

--dtype f32 (the default) measures the float32 handle and prints what this tool always printed.  With f16 or both the rows are
rounded to float16 first (and widened again for the f32 handle, the flat index and the centroids), so every handle holds the same
values.  f16 measures the float16 handle (lb_gpu_ivf_new_f16) alone.  both fills a float32 and a float16 handle in one process,
alternates their profiled runs, asserts that their labels and distances are equal in every cell, and prints per cell both
handles' four timing slots with the spread (min, max) of the scan slot, and the scan's bytes per second on each.

--dtype int8 rounds rows and queries into int8 (254 steps over [-0.5, 0.5)) and runs the int8 handle (lb_gpu_ivf_new_i8, int8
queries) beside the float32 handle over the same values widened, in one process, their profiled runs taking turns.  The two
handles' distances are different arithmetic (the reference's DataTypeInt8 kernels against its f32 chains), so what is asserted in
every cell is what must be equal: assignments, list sizes and search stats (the same lists probed).  For every nq the int8 handle
with every list probed is also asserted equal, labels and distances, to a flat int8 index over the same rows.
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
ELEM_BYTES = {"f32": 4, "f16": 2, "i8": 1}


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


def measured(steps, rows_scanned, dim, elem_bytes):
    """steps: [reps][4] ms of the profiled runs -> the medians of the four slots, the scan slot's spread and its rates"""
    med = np.median(np.asarray(steps, np.float64), axis=0)
    scan = [s[2] for s in steps]
    scan_bytes = rows_scanned * dim * elem_bytes
    return {"probes_ms": float(med[0]), "plan_ms": float(med[1]), "scan_ms": float(med[2]), "select_ms": float(med[3]),
            "scan_ms_min": float(min(scan)), "scan_ms_max": float(max(scan)), "bytes_scanned": scan_bytes,
            "scan_tb_per_s": scan_bytes / max(float(med[2]), 1e-6) / 1e9,
            "scan_share_of_8tb": scan_bytes / max(float(med[2]), 1e-6) * 1e3 / HBM_BYTES_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nprobe", type=int, nargs="*", default=[1, 8, 32, 256])
    ap.add_argument("--nq", type=int, nargs="*", default=[1, 8, 64, 1024])
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--dtype", choices=("f32", "f16", "both", "int8"), default="f32")
    ap.add_argument("--profile-reps", type=int, default=1, help="profiled searches per cell and handle (the slots are their medians)")
    a = ap.parse_args()
    lib = _lib.require_gpu(0)  # (raises without a GPU: nothing here falls back)
    out = {"rows": a.rows, "dim": a.dim, "nlist": a.nlist, "k": a.k, "dtype": a.dtype, "profile_reps": a.profile_reps,
           "shader_clock_mhz_before": clock_mhz(lib)}
    X = torch.empty((a.rows, a.dim), dtype=torch.float32, device="cuda")
    nqmax = max(a.nq)
    Q = torch.empty((nqmax, a.dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), a.rows * a.dim, 1, 0, None))
    _lib.check(lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), nqmax * a.dim, 2, 0, None))
    X16 = X8 = Q8 = None
    if a.dtype == "int8":  # int8 values: the float32 handle, the flat f32 index and the centroids see them widened
        X8 = (X * 254).round_().clamp_(-128, 127).to(torch.int8)
        Q8 = (Q * 254).round_().clamp_(-128, 127).to(torch.int8)
        X.copy_(X8)
        Q.copy_(Q8)
    elif a.dtype != "f32":  # fp16-representable rows: both handles, the flat index and the centroids see the same values
        X16 = X.to(torch.float16)
        X.copy_(X16)
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
    names = {"both": ("f32", "f16"), "int8": ("f32", "i8")}.get(a.dtype, (a.dtype,))
    pair = len(names) == 2
    other = names[-1]
    handles = {}
    for name in names:
        if name == "i8":
            h = ivf.IVFFlatInt8(cent)
        else:
            h = ivf.IVFFlat(cent, dtype=gpu.DataType.Float16 if name == "f16" else gpu.DataType.Float32)
        h.reserve(a.rows)
        t0 = time.perf_counter()
        h.add_device(a.rows, {"f16": X16, "i8": X8}.get(name, X).data_ptr())
        add_s = time.perf_counter() - t0
        handles[name] = h
        info = {"seconds": add_s, "rows_per_s": a.rows / add_s}
        if pair:
            out.setdefault("add", {})[name] = info
            out.setdefault("hbm_bytes", {})[name] = h.hbm_bytes
        else:
            out["add"], out["hbm_bytes"] = info, h.hbm_bytes
    first = handles[names[0]]
    sizes = first.list_sizes()
    if pair:
        assert np.array_equal(sizes, handles[other].list_sizes()), "the two handles' lists differ"
        X16 = None  # (the handle holds its own copy)
    flat8 = None
    if a.dtype == "int8":
        flat8 = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=a.dim, Metric=0, DataType=gpu.DataType.Int8))
        flat8.reserve(a.rows)
        flat8.add_device(a.rows, X8.data_ptr())
        X8 = None
    out["lists"] = {"min": int(sizes.min()), "median": int(np.median(sizes)), "max": int(sizes.max()), "empty": int((sizes == 0).sum())}

    flat = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=a.dim, Metric=0))
    flat.set_order(0)
    flat.reserve(a.rows)
    flat.add_device(a.rows, X.data_ptr())
    res = {name: (torch.empty((nqmax, a.k), dtype=torch.float32, device="cuda"), torch.empty((nqmax, a.k), dtype=torch.int64, device="cuda"))
           for name in names}
    FD = torch.empty((nqmax, a.k), dtype=torch.float32, device="cuda")
    FL = torch.empty((nqmax, a.k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cells = []
    for nq in a.nq:
        flat_ms = p50_ms(lambda: flat.search_device(nq, Q.data_ptr(), a.k, FD.data_ptr(), FL.data_ptr()))
        truth = FL[:nq].cpu().numpy()
        if flat8 is not None:  # every list probed: the flat int8 index, bit for bit
            D8, L8 = res["i8"]
            flat8.search_device(nq, Q8.data_ptr(), a.k, FD.data_ptr(), FL.data_ptr())
            handles["i8"].search_device(nq, Q8.data_ptr(), a.k, a.nlist, D8.data_ptr(), L8.data_ptr())
            assert torch.equal(L8[:nq], FL[:nq]), f"every list probed: labels differ from the flat int8 index at nq {nq}"
            assert torch.equal(D8[:nq], FD[:nq]), f"every list probed: distances differ from the flat int8 index at nq {nq}"
        for nprobe in a.nprobe:
            run = {name: (lambda h=handles[name], D=res[name][0], L=res[name][1]:
                          h.search_device(nq, (Q8 if h.dtype == 2 else Q).data_ptr(), a.k, nprobe, D.data_ptr(), L.data_ptr()))
                   for name in names}
            ms = {name: p50_ms(run[name]) for name in names}
            steps = {name: [] for name in names}
            for _ in range(max(1, a.profile_reps)):  # the handles take turns
                for name in names:
                    h = handles[name]
                    h.set_profiling(True)
                    run[name]()
                    h.set_profiling(False)
                    steps[name].append(h.last_timing())
            st = first.last_search_stats()
            got = res[names[0]][1][:nq].cpu().numpy()
            recall = float(np.mean([np.intersect1d(got[j], truth[j]).size / a.k for j in range(nq)]))
            cell = {"nq": nq, "nprobe": nprobe, "flat_p50_ms": flat_ms, "rows_scanned": st[1], "max_rows_per_query": st[2],
                    "selected_from_lds": st[3], "recall_at_k": recall}
            if a.dtype == "both":
                assert handles["f16"].last_search_stats() == st, f"search stats differ at nq {nq} nprobe {nprobe}"
                assert torch.equal(res["f32"][1][:nq], res["f16"][1][:nq]), f"labels differ at nq {nq} nprobe {nprobe}"
                assert torch.equal(res["f32"][0][:nq], res["f16"][0][:nq]), f"distances differ at nq {nq} nprobe {nprobe}"
                cell["equal"] = True
                for name in names:
                    cell[name] = dict(measured(steps[name], st[1], a.dim, ELEM_BYTES[name]), p50_ms=ms[name])
                cell["scan_f16_over_f32"] = cell["f16"]["scan_ms"] / max(cell["f32"]["scan_ms"], 1e-9)
            elif a.dtype == "int8":
                assert handles["i8"].last_search_stats() == st, f"search stats differ at nq {nq} nprobe {nprobe}"
                assert np.array_equal(handles["i8"].list_sizes(), sizes), f"list sizes differ at nq {nq} nprobe {nprobe}"
                assert np.array_equal(handles["i8"].assignments(), first.assignments()), f"assignments differ at nq {nq} nprobe {nprobe}"
                cell["equal_lists"] = cell["equal_flat_i8"] = True
                for name in names:
                    cell[name] = dict(measured(steps[name], st[1], a.dim, ELEM_BYTES[name]), p50_ms=ms[name])
                cell["scan_i8_over_f32"] = cell["i8"]["scan_ms"] / max(cell["f32"]["scan_ms"], 1e-9)
            else:
                m = measured(steps[names[0]], st[1], a.dim, ELEM_BYTES[names[0]])
                if a.profile_reps <= 1:
                    del m["scan_ms_min"], m["scan_ms_max"]
                cell.update(m, p50_ms=ms[names[0]])
            cells.append(cell)
    out["cells"] = cells
    out["shader_clock_mhz_after"] = clock_mhz(lib)
    print(json.dumps(out))
    flat.Close()
    if flat8 is not None:
        flat8.Close()
    for h in handles.values():
        h.Close()


if __name__ == "__main__":
    main()
