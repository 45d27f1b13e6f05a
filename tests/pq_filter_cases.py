"""Inputs and the two statements of a filtered ADC k-NN over PQ codes, shared by tests/test_pq_filter_semantics.py (CPU: the two
statements are shown to agree and the preconditions of the GPU cases are verified on the oracle) and
tests/test_gpu_pq_filters.py (GPU: the PQ handle is compared with the first statement on exactly these inputs).

The expected result is the C oracle on the visible subset (`subset_search`): vis = flatnonzero(mask), per query
adc_batch(build_adc_table(cb, q), codes[vis]) and topk_canonical over min(k, vis.size), labels mapped back through vis, the rest
-1 / FLT_MAX.  The independent statement (`masked_topk`) is the full ADC distance row with the hidden rows at +inf, a stable
argsort (ascending by (distance, row)) and its first k.

Masks come from tests/code_filter_cases.masks and tests/row_view_cases.  "Few code values": the bytes are drawn from four
values, so equal distances are common and the tie rule (the lowest rows win) is exercised."""
import functools
import os
import re

import numpy as np

from tests import row_view_cases as rv

F = np.float32
FLT_MAX = np.finfo(F).max
N = 5003                       # one boot chunk (the list's 8192 entries hold every position)
N_CHUNKS = 30_011              # case B: several chunks, no sampled plan
N_SAFE = 40_000                # case C
N_BIG = 200_003                # cases D, E, G: a 50 % mask leaves more than 65,536 rows (the sampled plan)
SHAPES = ((32, 16), (96, 48), (768, 96), (60, 5))   # (dims, M): aligned forms MCH 1 / 3 / 6 and the generic one
FEW = ((32, 16), (60, 5))      # shapes whose code bytes are drawn from four values
FEW_VALUES = np.array([3, 77, 128, 250], np.uint8)
BOOT_POSITIONS = 8192          # pq.hip: the boot chunk of a search with k <= 2048 (the whole 8192-entry list)


def list_waves():
    """waves per workgroup of the list kernels (lb_device.h): a workgroup walks runs of list_waves() * 64 positions"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "longbow_amd", "csrc", "lb_device.h")) as f:
        return int(re.search(r"constexpr int ADC_LIST_WAVES = (\d+);", f.read()).group(1))


def codebooks(rng, dims, M):
    return rng.random((M, 256, dims // M), dtype=F)


def codes_of(rng, n, M, few):
    if few:
        return FEW_VALUES[rng.integers(0, 4, (n, M))]
    return rng.integers(0, 256, (n, M), dtype=np.uint8)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def corpus(dims, M, n, nq=5, seed=0):
    """(codebooks, codes [n, M], queries [nq, dims]) of one shape and size: computed once, shared, never written to"""
    rng = np.random.default_rng(dims * 1000 + M + n + seed)
    cb = codebooks(rng, dims, M)
    codes = codes_of(rng, n, M, (dims, M) in FEW)
    Q = rng.random((nq, dims), dtype=F)
    return _frozen(cb, codes, Q)


def decode(cb, code):
    """the vector whose ADC distance to `code` is 0"""
    return np.concatenate([cb[j, code[j]] for j in range(cb.shape[0])]).astype(F)


# ---- the two statements --------------------------------------------------------------------------------------------------
def subset_search(oracle, cb, codes, Q, mask, k):
    """the oracle's ADC k-NN over the visible rows alone, labels mapped back to corpus rows -> (labels [nq, k], dist [nq, k])"""
    vis = np.flatnonzero(mask)
    Q = np.asarray(Q, F).reshape(-1, cb.shape[0] * cb.shape[2])
    labels = np.full((Q.shape[0], k), -1, np.int64)
    dist = np.full((Q.shape[0], k), FLT_MAX, F)
    have = min(k, vis.size)
    if have:
        sub = np.ascontiguousarray(codes[vis])
        for b, q in enumerate(Q):
            d = oracle.adc_batch(oracle.build_adc_table(cb, q), sub)
            oi, od, _ = oracle.topk_canonical(d, have)
            labels[b, :have] = vis[oi]
            dist[b, :have] = od
    return labels, dist


def masked_topk(oracle, cb, codes, Q, mask, k):
    """every row's ADC distance, the hidden rows at +inf, a stable argsort per query and its first k"""
    Q = np.asarray(Q, F).reshape(-1, cb.shape[0] * cb.shape[2])
    labels = np.full((Q.shape[0], k), -1, np.int64)
    dist = np.full((Q.shape[0], k), FLT_MAX, F)
    hidden = np.asarray(mask) == 0
    for b, q in enumerate(Q):
        d = oracle.adc_batch(oracle.build_adc_table(cb, q), codes).astype(np.float64)
        d[hidden] = np.inf
        order = np.argsort(d, kind="stable")[:k]
        ok = ~hidden[order]  # (an ADC distance may itself be +inf: visibility decides, not the value)
        labels[b, :order.size] = np.where(ok, order, -1)
        dist[b, :order.size] = np.where(ok, d[order], FLT_MAX).astype(F)
    return labels, dist


# ---- the cases -----------------------------------------------------------------------------------------------------------
def half_mask(n, seed=1):
    return rv.byte_mask(np.random.default_rng(n + seed), n, 0.5)


def third_mask(n):
    return (np.arange(n) % 3 != 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_c(M):
    """Safe schedule: the visible rows' ADC distances to the query strictly DECREASE with the row, so every position behind the
    boot chunk beats the threshold the boot chunk left.  sub = 1, query 0; table 0 is ~256 c, table 1 is ~c, the others 0; row r
    carries v = 65535 - r in its first two bytes, so its sum is ~v.  Every second row is hidden: 20,000 positions, of which the
    chunk behind the 8192-position boot chunk (chunk_end_host: it runs to the end) admits all 11,808 into an 8192-entry list."""
    cb = np.zeros((M, 256, 1), F)
    c = np.arange(256, dtype=F)
    cb[0, :, 0] = F(16) * np.sqrt(c)
    cb[1, :, 0] = np.sqrt(c)
    v = 65535 - np.arange(N_SAFE)
    codes = np.zeros((N_SAFE, M), np.uint8)
    codes[:, 0] = v >> 8
    codes[:, 1] = v & 255
    Q = np.zeros((2, M), F)
    mask = (np.arange(N_SAFE) % 2 == 0).astype(np.uint8)
    return _frozen(cb, codes, Q, mask)


@functools.lru_cache(maxsize=None)
def case_e():
    """Ties at the sampled plan's size: 50 distinct code rows repeated over N_BIG rows"""
    dims, M = 32, 16
    rng = np.random.default_rng(50)
    cb = codebooks(rng, dims, M)
    base = codes_of(rng, 50, M, True)
    codes = np.ascontiguousarray(base[np.arange(N_BIG) % 50])
    Q = rng.random((3, dims), dtype=F)
    return _frozen(cb, codes, Q, half_mask(N_BIG, 5))


@functools.lru_cache(maxsize=None)
def case_f(dims, M, boundary):
    """Duplicates across a boundary of the list: the 12 visible rows at list positions boundary - 6 .. boundary + 5 and the
    hidden rows between them all carry the code whose decoded vector is query 0 (distance 0).  Codes over the whole byte range
    here, so that no other row equals it.  -> (cb, codes, Q, mask, block)"""
    rng = np.random.default_rng(dims + M + boundary)
    cb = codebooks(rng, dims, M)
    codes = codes_of(rng, N, M, False)
    mask = third_mask(N)
    vis = np.flatnonzero(mask)
    block = vis[boundary - 6:boundary + 6]
    near = codes_of(rng, 1, M, False)[0]
    codes[block[0]:block[-1] + 1] = near
    Q = np.stack([decode(cb, near), rng.random(dims, dtype=F), rng.random(dims, dtype=F)])
    return _frozen(cb, codes, Q, mask, block)


@functools.lru_cache(maxsize=None)
def case_g():
    """The degenerate tables of tests/test_gpu_pq.py::test_prefilter_degenerate_tables under a 50 % mask: constant sub-tables
    (every distance ties, every row survives the byte bound and overflows the candidate buffer) and a query with an infinite
    component (the prefilter is refused on the device).  -> (zero codebooks, random codebooks, codes, Q = [q, qbad], mask)"""
    rng = np.random.default_rng(5)
    M, dims = 16, 64
    cb0 = np.zeros((M, 256, dims // M), F)
    codes = rng.integers(0, 256, (N_BIG, M), dtype=np.uint8)
    q = rng.random(dims, dtype=F)
    cb = rng.random((M, 256, dims // M), dtype=F)
    qbad = q.copy()
    qbad[3] = np.inf
    return _frozen(cb0, cb, codes, np.stack([q, qbad]), half_mask(N_BIG, 7))
