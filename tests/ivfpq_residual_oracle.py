"""The residual form of the IVF-PQ semantics of include/longbow_gpu.h (lb_gpu_ivfpq_new_residual) restated over
tests/ivfpq_oracle.py, tests/ivf_oracle.py and the C oracle: the lists are the plain handle's, the code of a row is pq_encode of
the f32 difference of the row and its list's centroid, and a query has an ADC table per probed list, build_adc_table of the f32
difference of the query and that list's centroid; the result is topk_canonical over the rows of the probed lists, ascending.
Also the pure host rules of the residual search (lb_ivfpq.h), so that CPU tests pin them.  The shared inputs are
tests/ivfpq_oracle.py's."""
import numpy as np

from tests import ivf_oracle as io
from tests import ivfpq_oracle as pqo

F = np.float32
FLT_MAX = pqo.FLT_MAX
TILE, GRID = pqo.TILE, pqo.GRID
TABLE_SCRATCH = 1 << 30  # kTableScratch: bytes of tables a batch may hold
QUERY_BATCH = 1024       # kQueryBatch


def residuals(X, C, lists):
    """res(x, l)[i] = x[i] - C[l][i]: one f32 subtraction a component"""
    return (np.asarray(X, F) - np.asarray(C, F)[np.asarray(lists)]).astype(F)


def encode(oracle, cb, X, C, lists):
    """the codes of a residual handle: pq_encode of every row's residual to its list's centroid"""
    return pqo.encode(oracle, cb, residuals(X, C, lists))


def search(oracle, cb, order, Q, C, lists, codes, k, nprobe, ids=None, visible=None):
    """-> (labels [nq, k], dist [nq, k], rows scanned per query [nq]); visible: a mask over the rows (non-zero: visible)"""
    lists = np.asarray(lists)
    if visible is not None:
        lists = np.where(np.asarray(visible) != 0, lists, -1)  # a hidden row is a row in no list
    nq = Q.shape[0]
    labels = np.empty((nq, k), np.int64)
    dist = np.empty((nq, k), F)
    scanned = np.empty(nq, np.int64)
    for j in range(nq):
        pr = io.probes(oracle, 0, order, Q[j], C, nprobe)
        rows = io.probed_rows(lists, pr)
        scanned[j] = rows.size
        if rows.size == 0:
            labels[j], dist[j] = -1, FLT_MAX
            continue
        d = np.empty(rows.size, F)
        of = lists[rows]
        for l in pr:  # a table per probed list
            sel = of == l
            if sel.any():
                table = oracle.build_adc_table(cb, (Q[j] - C[l]).astype(F))
                d[sel] = oracle.adc_batch(table, codes[rows[sel]])
        oi, od, _ = oracle.topk_canonical(d, k)
        lab = np.where(oi >= 0, rows[np.clip(oi, 0, rows.size - 1)], -1).astype(np.int64)
        if ids is not None:
            lab = np.where(lab >= 0, ids[np.clip(lab, 0, None)], -1)
        labels[j], dist[j] = lab, od
    return labels, dist, scanned


def rscan_groups(pairs, maxlen):
    """ivfpq_rscan_groups (lb_ivfpq.h): workgroups per pair (query, probed list) of the residual scan"""
    return max(1, min(-(-GRID // pairs), -(-maxlen // TILE)))


RUN_MAX = 8  # IPQ_RUN_MAX: tiles per item of the scan's work list at most


def rscan_plan(pairs, nq, pmax, maxlen):
    """ivfpq_rscan_plan (lb_ivfpq.h) -> ("strided", G), while the longest list is at most two steps of a pair's G workgroups, or
    ("items", tiles per item, workgroups launched): the work list"""
    G, tiles_max = rscan_groups(pairs, maxlen), -(-maxlen // TILE)
    if tiles_max <= 2 * G:
        return ("strided", G)
    tiles = pairs + -(-(nq * pmax) // TILE)
    run = max(1, min(RUN_MAX, -(-tiles // GRID)))
    return ("items", run, pairs + -(-tiles // run))


def table_plan(np_, M, budget=TABLE_SCRATCH):
    """ivfpq_table_plan (lb_ivfpq.h) -> (queries per batch at most, slots of a query per round): nb * np tables of M * 1024
    bytes fit the budget; only when one query's np tables do not, one query a batch and rounds of as many slots as fit"""
    fit = max(1, budget // (M * 1024))
    return (fit // np_, np_) if np_ <= fit else (1, fit)


def batch_queries(nq, np_, M):
    """queries of a residual search's batch where the keys set no tighter bound"""
    return min(nq, QUERY_BATCH, table_plan(np_, M)[0])


def slot_rounds(np_, M):
    slots = table_plan(np_, M)[1]
    return -(-np_ // slots)


ZERO_CENTROIDS = (0.0, 1e6, -1e6)  # in every coordinate: every standard-normal row lands in list 0, whose centroid is zero


def zero_centroid_case(dims=16, M=4, n=2000, nq=20):
    """parity rows and queries under centroids (0, +1e6, -1e6): the residual of every row is the row"""
    X, Q, _, cb = pqo.parity_case(dims, M, n=n, nq=nq)
    C = np.stack([np.full(dims, v, F) for v in ZERO_CENTROIDS])
    return X, Q, C, cb


def clustered_case(seed=3, n=4000, dims=32, nlist=16, nq=40, spread=3.0):
    """rows centres[owner] + unit noise, centres spread * N(0, 1); queries drawn the same way"""
    rng = np.random.default_rng(seed)
    centres = (F(spread) * rng.standard_normal((nlist, dims))).astype(F)
    X = (centres[rng.integers(0, nlist, n)] + rng.standard_normal((n, dims)).astype(F)).astype(F)
    Q = (centres[rng.integers(0, nlist, nq)] + rng.standard_normal((nq, dims)).astype(F)).astype(F)
    return X, Q
