"""numpy restatement of the ADC search planner and of adc_quantise_kernel (kernels_pq2.hip), the same float32
operations in the same order.  Test infrastructure: tests/test_adc_bound_semantics.py checks the premise of the
byte-table prefilter with it on the CPU, tests/test_gpu_pq_forms.py derives from it what the device must do."""
import math

import numpy as np

F = np.float32
CAND_CAP = 65536              # pq.hip: kCandCap
MIN_RANGE = F(2.0 ** -100)    # kernels_pq2.hip: kAdcMinRange
FLT_MAX = np.finfo(F).max


def next_pow2(v):
    p = 2
    while p < v:
        p <<= 1
    return p


def plan(n, k):
    """pq.hip's sample_plan, the sampled-threshold plan of a PQ search -> (samp_count, m, stride, cap); samp_count 0 = bootstrap"""
    cap = max(8192, 4 * next_pow2(k))
    if 65536 <= n < (1 << 32):
        cap_s = max(16384, cap)
        stride = 512 if n >= 8192 * 512 else 256
        cnt = max(8192, (n + stride - 1) // stride)
        lam = k * cnt / n
        m = max(8, math.ceil(lam + 5.0 * math.sqrt(lam) + 4.0))
        loose = m * (n / cnt) * (1.0 + 5.0 / math.sqrt(m))
        if m <= 32 and loose <= cap_s - k and cnt <= 8192 * (8192 // m):
            return cnt, m, stride, cap_s
    return 0, 0, 0, cap


def sample_rows(n, cnt):
    """adc_sample_kernel: row of sample i = floor(i * n / cnt)"""
    return (np.arange(cnt, dtype=np.uint64) * np.uint64(n) // np.uint64(cnt)).astype(np.int64)


def sampled_tau(dist, cnt, m):
    """the m-th smallest (with multiplicity) distance of the sampled rows; rows with dist <= it are admitted
    (sample_tau_kernel saturates the row bits of the threshold entry)"""
    s = np.sort(dist[sample_rows(dist.size, cnt)])
    return F(s[m - 1])


def minrng(table):
    """build_adc_table_kernel's per-subtable {min, max - min, bad}; table is [M, 256] float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        mn = np.fmin.reduce(table, axis=1).astype(F)
        mx = np.fmax.reduce(table, axis=1).astype(F)
        rng = (mx - mn).astype(F)
        bad = (~(table >= 0) | (table > F(3.0e38))).any(axis=1)
    return mn, rng, bad


def quantise(table, tau_dist, floor=MIN_RANGE):
    """adc_quantise_kernel: byte table [M, 256] and (s_tau, ok).  floor=None restates the arithmetic without the
    range floor (the kernel before the floor existed)."""
    table = np.ascontiguousarray(table, F)
    M = table.shape[0]
    mn, rng, bad = minrng(table)
    rmax = F(0)
    for r in rng:                                # fmaxf ignores NaN
        if r > rmax:
            rmax = F(r)
    base = float(np.sum(mn.astype(np.float64)))
    with np.errstate(all="ignore"):
        s_scale = F(rmax / F(255)) if rmax > 0 else F(1)
        s_inv = F(F(255) / rmax) if rmax > 0 else F(0)
        r = ((table - mn[:, None]).astype(F) * s_inv).astype(F)
        fl = np.floor(r)
    # the device's float -> int conversion gives 0 for NaN and saturates at the ends
    q = np.clip(np.nan_to_num(fl, nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.uint8)
    ok = 0 if bad.any() else 1
    if floor is not None and (not np.isfinite(s_inv) or (rmax > 0 and rmax < floor)):
        ok = 0
    s_tau = 0
    td = F(tau_dist)
    if not (td >= 0) or td > F(1.0e18):
        ok = 0
    else:
        tn = (F(td + F(0)).view(np.uint32) + np.uint32(1)).view(F)
        U = float(tn) * float(tn)
        gamma = 1.05 * M * 5.9604644775390625e-8
        lim = (U * (1.0 + 2.0 * gamma) - base) / float(s_scale) + 2.0
        if lim < 0.0:
            s_tau = -1
        elif lim > 2.0e9:
            ok = 0
        else:
            s_tau = int(lim)
    return q, s_tau, ok


def byte_sums(q, codes):
    """S = sum_j q[j][codes[row][j]] for every row"""
    M = q.shape[0]
    S = np.zeros(codes.shape[0], np.int64)
    for j in range(M):
        S += q[j][codes[:, j]]
    return S


def family(name, M, sub, rng):
    """codebooks [M, 256, sub] and one query of the issue's table families"""
    cb = rng.random((M, 256, sub), dtype=F)
    q = rng.random(M * sub, dtype=F)
    if name == "dominant":      # one subspace scaled by 100: 1e4 in its subtable
        cb[M // 2] *= F(100)
        q[(M // 2) * sub:(M // 2 + 1) * sub] *= F(100)
    elif name == "offset":      # large base, small range
        q = (q + F(1000)).astype(F)
    elif name == "dyadic":      # (t - min) / s lands on integers
        cb = (rng.integers(0, 17, (M, 256, sub)) / 16.0).astype(F)
        q = (rng.integers(0, 17, M * sub) / 16.0).astype(F)
    elif name == "huge":        # table entries near 1e30
        cb, q = (cb * F(1e15)).astype(F), (q * F(1e15)).astype(F)
    elif name == "tiny":        # table entries at and below 7.5e-37
        cb, q = (cb * F(1e-19)).astype(F), (q * F(1e-19)).astype(F)
    return cb, q


def wrong_survivor_corpus(n, M=16, sub=2):
    """Tiny-magnitude corpus on which the bound without the floor returns a WRONG list instead of an empty one.
    Query 0; per subspace centroid 0 is the nearest (|c|^2 = 1e-38), centroid 1 just above it, centroid 2 the farthest
    (9e-38), the others between.  Rows: five whose every code is 1 (the true nearest; S = 255 M once 255 / rmax = inf),
    one row in 32 with a single farthest entry and minima elsewhere (S = 255), fillers of codes >= 3."""
    rng = np.random.default_rng(4242)
    s = F(1e-19)
    cb = np.zeros((M, 256, sub), F)
    cb[:, :, 0] = (F(1.5) + rng.random((M, 256), dtype=F) * F(1.4)) * s
    cb[:, 0, 0], cb[:, 1, 0], cb[:, 2, 0] = s, F(1.01) * s, F(3) * s
    codes = rng.integers(3, 256, (n, M), dtype=np.uint8)
    ring = np.arange(3, n, 32)
    codes[ring] = 0
    codes[ring, ring % M] = 2
    near = np.array([1000, 20001, 30002, 40005, 50007])
    codes[near] = 1
    return cb, np.zeros(M * sub, F), codes, near
