"""The IVF-PQ semantics of include/longbow_gpu.h (lb_gpu_ivfpq_*) restated over what the suite already trusts: the lists are
tests/ivf_oracle.py's at metric 0 (L2), the codes the C oracle's pq_encode, the distances its build_adc_table + adc_batch and the
result its topk_canonical over the rows of the probed lists.  Also the inputs the CPU and the GPU tests share, so that what
tests/test_ivfpq_semantics.py asserts of them holds for tests/test_gpu_ivfpq.py."""
import struct

import numpy as np

from tests import ivf_oracle as io

F = np.float32
FLT_MAX = np.finfo(F).max
TILE = 1024  # IPQ_TILE: positions per tile of the scan
GRID = 512   # IPQ_GRID: workgroups a scan launch aims at


def scan_groups(nq, pmax):
    """ivfpq_scan_groups (lb_ivfpq.h): workgroups per query of the scan"""
    return max(1, min(-(-pmax // TILE), -(-GRID // nq)))


def codebooks(dims, M, seed):
    """standard-normal codebooks [M, 256, dims / M]: the scale of the standard-normal rows of the cases below"""
    return np.random.default_rng(seed).standard_normal((M, 256, dims // M)).astype(F)


def blob(cb):
    """PQEncoder.Serialize (persistence.go:9-35)"""
    M, K, sub = cb.shape
    return struct.pack("<III", M * sub, M, K) + np.ascontiguousarray(cb, "<f4").tobytes()


def encode(oracle, cb, X):
    codes = np.empty((X.shape[0], cb.shape[0]), np.uint8)
    for i in range(X.shape[0]):
        codes[i] = oracle.pq_encode(cb, X[i])
    return codes


def assign(oracle, order, X, C):
    return io.assign(oracle, 0, order, X, C)


def _topk(oracle, cb, q, codes, rows, k, ids):
    """canonical top-k of one query over codes[rows] (rows ascending) -> (labels [k], dist [k]), padded -1 / FLT_MAX"""
    if rows.size == 0:
        return np.full(k, -1, np.int64), np.full(k, FLT_MAX, F)
    d = oracle.adc_batch(oracle.build_adc_table(cb, q), codes[rows])
    oi, od, _ = oracle.topk_canonical(d, k)
    lab = np.where(oi >= 0, rows[np.clip(oi, 0, rows.size - 1)], -1).astype(np.int64)
    if ids is not None:
        lab = np.where(lab >= 0, ids[np.clip(lab, 0, None)], -1)
    return lab, od


def search(oracle, cb, order, Q, C, lists, codes, k, nprobe, ids=None):
    """-> (labels [nq, k], dist [nq, k], rows scanned per query [nq])"""
    labels = np.empty((Q.shape[0], k), np.int64)
    dist = np.empty((Q.shape[0], k), F)
    scanned = np.empty(Q.shape[0], np.int64)
    for j in range(Q.shape[0]):
        rows = io.probed_rows(lists, io.probes(oracle, 0, order, Q[j], C, nprobe))
        scanned[j] = rows.size
        labels[j], dist[j] = _topk(oracle, cb, Q[j], codes, rows, k, ids)
    return labels, dist, scanned


def brute(oracle, cb, Q, codes, k):
    """the ADC top-k over every code: what lb_gpu_pq_search returns"""
    labels = np.empty((Q.shape[0], k), np.int64)
    dist = np.empty((Q.shape[0], k), F)
    rows = np.arange(codes.shape[0])
    for j in range(Q.shape[0]):
        labels[j], dist[j] = _topk(oracle, cb, Q[j], codes, rows, k, None)
    return labels, dist


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
PARITY_SHAPES = ((16, 4), (32, 16))  # (dims, M): the byte form and the 16-byte form of the scan


def parity_case(dims, M, n=3000, nlist=16, nq=33):
    X, Q, C = io.parity_case(n, dims, nlist, nq, seed=1234 + M)
    return X, Q, C, codebooks(dims, M, 4321 + M)


# lists of 0, 1, TILE - 1, TILE, TILE + 1 rows, one longer than G * TILE at the 66 queries of edge_case (G = 8), and short ones
# that leave several list boundaries inside one wave's 64 positions
EDGE_COUNTS = (0, 1, TILE - 1, TILE, TILE + 1, 8 * TILE + 77, 3, 5, 2, 0, 7)
EDGE_LONG = 5


def edge_case():
    """ivf_oracle.edge_case's way of forcing the counts (centroids 100 e_i, rows their centroid plus unit noise, so that the
    codes of a list differ), and 66 queries: six near every centroid"""
    X, Q, C, owner = io.edge_case(EDGE_COUNTS, dim=16, seed=5, noise=1.0)
    rng = np.random.default_rng(55)
    Q = np.concatenate([Q] + [(C + rng.standard_normal(C.shape).astype(F)).astype(F) for _ in range(5)])
    return X, Q, C, owner, codebooks(16, 4, 99)


def skew_case():
    """ivf_oracle.skew_case: a list beyond what a selection holds in LDS; dims 8, M 4"""
    X, Q, C = io.skew_case()
    return X, Q, C, codebooks(8, 4, 78)
