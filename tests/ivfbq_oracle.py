"""The IVF-BQ semantics of include/longbow_gpu.h (lb_gpu_ivfbq_*) restated over what the suite already trusts: the lists and
probes are tests/ivf_oracle.py's at metric 0 (L2), the codes tests/bq_oracle.py's encode, the distances its hamming and the
result its topk (ascending (h, position), reported as float32(h)) over the rows of the probed lists.  Also the inputs the CPU
and the GPU tests share, so that what tests/test_ivfbq_semantics.py asserts of them holds for tests/test_gpu_ivfbq.py."""
import numpy as np

from tests import bq_oracle as bo
from tests import ivf_oracle as io

F = np.float32
FLT_MAX = np.finfo(F).max
TILE = 256       # IBQ_ROWS: rows per tile of the scan == lanes of a workgroup
GRID = 4096      # workgroups a scan launch aims at (launch_ivfbq_scan, as launch_ivf_scan)
LDS_KEYS = 16384  # IVF_SELECT_LDS_KEYS: a query with more scanned rows is selected from global memory


def chunk_words(W):
    """the chunk rule of the scan (ibq_cw, as bq_cw): words of each row per LDS stage"""
    return 4 if W <= 4 else 8 if W <= 8 else 12 if W <= 12 else 16 if W <= 16 else 8


def chunks(W):
    """stages a tile of W-word rows takes"""
    return -(-W // chunk_words(W))


def scan_tiles_x(pairs, maxlen):
    """launch_ivfbq_scan's grid.x: workgroups along one list; each walks tiles x, x + grid.x, ... of it"""
    return max(1, min(-(-maxlen // TILE), max(1, -(-GRID // pairs))))


def assign(oracle, order, X, C):
    return io.assign(oracle, 0, order, X, C)


def encode(X):
    return bo.encode(X)


def _topk(qcode, codes, rows, k, ids):
    """top-k of one query code over codes[rows] (rows ascending) -> (labels [k], dist [k]), padded -1 / FLT_MAX"""
    lab, d = bo.topk(bo.hamming(qcode, codes[rows]) if rows.size else np.zeros(0, np.int32), k)
    if rows.size:  # (else all padding already)
        lab = np.where(lab >= 0, rows[np.clip(lab, 0, rows.size - 1)], -1).astype(np.int64)
    if ids is not None:
        lab = np.where(lab >= 0, ids[np.clip(lab, 0, None)], -1)
    return lab, d


def search(oracle, order, Q, C, lists, codes, k, nprobe, ids=None, mask=None):
    """-> (labels [nq, k], dist [nq, k], rows scanned per query [nq]); mask (uint8 [n], optional): the row filter"""
    qc = bo.encode(Q)
    labels = np.empty((Q.shape[0], k), np.int64)
    dist = np.empty((Q.shape[0], k), F)
    scanned = np.empty(Q.shape[0], np.int64)
    for j in range(Q.shape[0]):
        rows = io.probed_rows(lists, io.probes(oracle, 0, order, Q[j], C, nprobe))
        if mask is not None:
            rows = rows[np.asarray(mask)[rows] != 0]
        scanned[j] = rows.size
        labels[j], dist[j] = _topk(qc[j], codes, rows, k, ids)
    return labels, dist, scanned


def brute(Q, codes, k):
    """the top-k over every code: what lb_gpu_bq_search returns"""
    return bo.search(bo.encode(Q), codes, k)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
# W = 1 with pad bits (a chunk of 4 with three zero words); W = 2 with pad bits; the workload's 12-word single chunk; the 16-word
# boundary of the single chunk; 17 words: two chunks of 8 plus a partial one
PARITY_DIMS = (16, 100, 768, 1024, 1088)


def parity_case(dims, n=3000, nlist=16, nq=33):
    """ivf_oracle.parity_case -> X, Q, C"""
    return io.parity_case(n, dims, nlist, nq, seed=4321 + dims)


def tie_case():
    """dims 16: a distance takes 17 values.  The rows of ivf_oracle.parity_case three times over, at a seed for which the top 10
    of every query holds a tie group whose rows lie in more than one list (tests/test_ivfbq_semantics.py asserts it)
    -> X3, Q, C"""
    X, Q, C = io.parity_case(3000, 16, 16, 33, seed=101)
    return np.concatenate((X, X, X)), Q, C


# lists of 0, 1, TILE - 1, TILE, TILE + 1 rows, one longer than grid.x * TILE at the 264 queries of edge_case with one probe
# (grid.x = 16 against 18 tiles), and short ones that leave several list boundaries inside one wave's 64 positions
EDGE_COUNTS = (0, 1, TILE - 1, TILE, TILE + 1, 17 * TILE + 77, 3, 5, 2, 0, 7)
EDGE_LONG = 5
EDGE_PER_LIST = 24  # queries near every centroid


def edge_case():
    """ivf_oracle.edge_case's way of forcing the counts (centroids 100 e_i, rows their centroid plus unit noise, so that the
    codes of a list differ), 24 queries near every centroid (query i probes list i % nlist first) -> X, Q, C, owner"""
    X, Q, C, owner = io.edge_case(EDGE_COUNTS, dim=16, seed=5, noise=1.0)
    rng = np.random.default_rng(55)
    Q = np.concatenate([Q] + [(C + rng.standard_normal(C.shape).astype(F)).astype(F) for _ in range(EDGE_PER_LIST - 1)])
    return X, Q, C, owner


def skew_case():
    """ivf_oracle.skew_case: a list beyond what a selection holds in LDS; dims 8 -> X, Q, C"""
    return io.skew_case()
