"""The IVF-SQ8 semantics of include/longbow_gpu.h (lb_gpu_ivfsq8_*) restated over what the suite already trusts: the lists and
probes are tests/ivf_oracle.py's at metric 0 (L2), the codes tests/sq8_oracle.py's encode, the distances its dist_s and the
result its topk (ascending (S, position) of the integers, reported as float32(S)) over the rows of the probed lists.  Also the
inputs the CPU and the GPU tests share, so that what tests/test_ivfsq8_semantics.py asserts of them holds for
tests/test_gpu_ivfsq8.py."""
import numpy as np

from tests import ivf_oracle as io
from tests import sq8_oracle as so

F = np.float32
FLT_MAX = np.finfo(F).max
TILE = 128       # ISQ_ROWS: rows per tile of the scan == lanes of a workgroup
GRID = 4096      # workgroups a scan launch aims at (launch_ivfsq8_scan, as launch_ivf_scan)
LDS_KEYS = 16384  # IVF_SELECT_LDS_KEYS: a query with more scanned rows is selected from global memory


def scan_tiles_x(pairs, maxlen):
    """launch_ivfsq8_scan's grid.x: workgroups along one list; each walks tiles x, x + grid.x, ... of it"""
    return max(1, min(-(-maxlen // TILE), max(1, -(-GRID // pairs))))


def assign(oracle, order, X, C):
    return io.assign(oracle, 0, order, X, C)


def encode(X, mn, mx):
    return so.encode(X, mn, mx)


def _topk(qcode, codes, rows, k, ids):
    """top-k of one query code over codes[rows] (rows ascending) -> (labels [k], dist [k]), padded -1 / FLT_MAX"""
    lab, d = so.topk(so.dist_s(qcode, codes[rows]), k)
    if rows.size:  # (else all padding already)
        lab = np.where(lab >= 0, rows[np.clip(lab, 0, rows.size - 1)], -1).astype(np.int64)
    if ids is not None:
        lab = np.where(lab >= 0, ids[np.clip(lab, 0, None)], -1)
    return lab, d


def search(oracle, order, Q, C, lists, codes, mn, mx, k, nprobe, ids=None, mask=None):
    """-> (labels [nq, k], dist [nq, k], rows scanned per query [nq]); mask (uint8 [n], optional): the row filter"""
    qc = so.encode(Q, mn, mx)
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


def brute(Q, codes, mn, mx, k):
    """the top-k over every code: what lb_gpu_sq8_search returns"""
    return so.search(so.encode(Q, mn, mx), codes, k)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
CHUNK = 8  # ISQ_CH: 16-byte pieces of a row per stage of the scan
# one 16-byte piece; a padded stride (32 bytes for 20); 80: five pieces, a partial chunk alone; 144: one full chunk of eight
# pieces plus a partial one; the workload's row: six full chunks
PARITY_DIMS = (16, 20, 80, 144, 768)


def parity_case(dims, n=3000, nlist=16, nq=33):
    """ivf_oracle.parity_case plus the bounds of sq8_oracle.train(X) -> X, Q, C, min, max"""
    X, Q, C = io.parity_case(n, dims, nlist, nq, seed=1234 + dims)
    mn, mx = so.train(X)
    return X, Q, C, mn, mx


# lists of 0, 1, TILE - 1, TILE, TILE + 1 rows, one longer than grid.x * TILE at the 264 queries of edge_case with one probe
# (grid.x = 16), and short ones that leave several list boundaries inside one wave's 64 positions
EDGE_COUNTS = (0, 1, TILE - 1, TILE, TILE + 1, 17 * TILE + 77, 3, 5, 2, 0, 7)
EDGE_LONG = 5
EDGE_PER_LIST = 24  # queries near every centroid


def edge_case():
    """ivf_oracle.edge_case's way of forcing the counts (centroids 100 e_i, rows their centroid plus unit noise, so that the
    codes of a list differ), 24 queries near every centroid (query i probes list i % nlist first), bounds trained on the rows
    -> X, Q, C, owner, min, max"""
    X, Q, C, owner = io.edge_case(EDGE_COUNTS, dim=16, seed=5, noise=1.0)
    rng = np.random.default_rng(55)
    Q = np.concatenate([Q] + [(C + rng.standard_normal(C.shape).astype(F)).astype(F) for _ in range(EDGE_PER_LIST - 1)])
    mn, mx = so.train(X)
    return X, Q, C, owner, mn, mx


def skew_case():
    """ivf_oracle.skew_case: a list beyond what a selection holds in LDS; dims 8 -> X, Q, C, min, max"""
    X, Q, C = io.skew_case()
    mn, mx = so.train(X)
    return X, Q, C, mn, mx


ROUNDING_S = (16777217, 16777216, 16777217, 16777216)


def rounding_case():
    """Two S above 2^24 that round to one float.  dims 264, bounds 0 / 255 (scale exactly 1: integer-valued rows encode to
    themselves), the query all zeros.  Row B = 258 x 255, then 27, 6, 1, rest 0: S = 2^24; row A = B with one more 1:
    S = 2^24 + 1.  Rows [A, B, A, B]; two far-apart centroids -> X, Q, C, min, max"""
    dims = 264
    B = np.zeros(dims, F)
    B[:258] = 255
    B[258:261] = (27, 6, 1)
    A = B.copy()
    A[261] = 1
    X = np.stack((A, B, A, B)).astype(F)
    Q = np.zeros((1, dims), F)
    C = np.stack((np.zeros(dims, F), np.full(dims, 1000, F)))
    return X, Q, C, np.zeros(dims, F), np.full(dims, 255, F)
