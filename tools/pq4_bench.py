#!/usr/bin/env python3
"""PQ4 against PQ (K = 256) on one MI355X: exact ADC k-NN over N x 768 vectors' codes, wall clock around search_device
(which ends in a stream synchronise), median of the timed repeats, the variants alternated within each repeat.

  pq4_m96     PQ4Encoder, M = 96   (48 bytes a row), as it searches by default (tables in LDS, two queries a pass)
  pq4_m96_reg the same handle with the tables in registers, four queries a pass (the diagnostic build's LB_PQ4_LOOKUP=0):
              the lookup A/B of DESIGN
  pq4_m192   PQ4Encoder, M = 192  (96 bytes a row; tables in LDS)
  pq_m96     PQEncoder (K = 256), M = 96 (96 bytes a row), as it searches by default

usage: python tools/pq4_bench.py [N_millions=1] -> profiles/pq4_bench.json"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from longbow_amd import _lib, pq, pq4

N = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 1_000_000
D, K_NN, BATCHES = 768, 100, (1, 64, 1024)
lib = _lib.load_diag()
if lib.lb_gpu_device_count() <= 0:
    raise SystemExit("no GPU: nothing is measured")


def handle(cls, M, K):
    cb = torch.empty((M, K, D // M), device="cuda")
    lib.lb_gpu_fill_uniform_device(0, cb.data_ptr(), cb.numel(), 7 + M + K, 0, None)
    enc = cls(pq.serialize_codebooks(cb.cpu().numpy()), lib=lib)
    codes = torch.empty((N, M), dtype=torch.uint8, device="cuda")
    lib.lb_gpu_fill_codes_device(0, codes.data_ptr(), codes.numel(), 99, 0, None)
    if K == 16:
        codes &= 15
    enc.add_codes_device(N, codes.data_ptr())
    return enc


def lookup(v):
    os.environ["LB_PQ4_LOOKUP"] = v  # -1: the library's own choice


e96, e192, e256 = handle(pq4.PQ4Encoder, 96, 16), handle(pq4.PQ4Encoder, 192, 16), handle(pq.PQEncoder, 96, 256)
variants = [("pq4_m96", e96, "-1"), ("pq4_m96_reg", e96, "0"), ("pq4_m192", e192, "-1"), ("pq_m96", e256, "-1")]
row_bytes = {"pq4_m96": 48, "pq4_m96_reg": 48, "pq4_m192": 96, "pq_m96": 96}
out = {"n": N, "dims": D, "k": K_NN, "bytes_per_row": row_bytes, "ms_per_batch": {}, "ratio_pq4_m96_over_pq_m96": {},
       "ratio_reg_over_lds_lookup_m96": {}}
for nq in BATCHES:
    Q = torch.empty((nq, D), device="cuda")
    lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), Q.numel(), 42, 0, None)
    od = torch.empty((nq, K_NN), device="cuda")
    ol = torch.empty((nq, K_NN), dtype=torch.int64, device="cuda")
    reps = 40 if nq == 1 else 12 if nq == 64 else 5
    ts = {name: [] for name, _, _ in variants}
    res = {}
    for r in range(reps + 2):  # two warm-up rounds
        for name, enc, mode in variants:
            lookup(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc.search_device(nq, Q.data_ptr(), K_NN, od.data_ptr(), ol.data_ptr())
            dt = time.perf_counter() - t0
            if r >= 2:
                ts[name].append(dt)
            elif r == 0:
                res[name] = (ol.cpu().numpy().copy(), od.cpu().numpy().copy())
    lookup("-1")
    assert all(np.array_equal(a, b) for a, b in zip(res["pq4_m96"], res["pq4_m96_reg"])), "the two lookups disagree"
    med = {name: float(np.median(v)) * 1e3 for name, v in ts.items()}
    spread = {name: [float(np.min(v)) * 1e3, float(np.max(v)) * 1e3] for name, v in ts.items()}
    out["ms_per_batch"][str(nq)] = {"median": med, "min_max": spread, "repeats": reps}
    out["ratio_pq4_m96_over_pq_m96"][str(nq)] = med["pq4_m96"] / med["pq_m96"]
    out["ratio_reg_over_lds_lookup_m96"][str(nq)] = med["pq4_m96_reg"] / med["pq4_m96"]
    print(f"nq={nq}: " + ", ".join(f"{n} {m:.3f} ms" for n, m in med.items()), flush=True)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "pq4_bench.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out["ratio_pq4_m96_over_pq_m96"]), json.dumps(out["ratio_reg_over_lds_lookup_m96"]))
