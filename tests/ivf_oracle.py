"""The IVF-Flat semantics of include/longbow_gpu.h (lb_gpu_ivf_*) restated over what the suite already trusts: the C oracle's
batch_flat (the reference's distance arithmetic) and topk_canonical (ascending (distance, position), NaN last).  Also the inputs
the CPU and the GPU tests share, so that what tests/test_ivf_semantics.py asserts of them holds for tests/test_gpu_ivf.py."""
import numpy as np

from tests.gpu_util import oracle_topk_rows_parallel

F = np.float32
FLT_MAX = np.finfo(F).max


def assign(oracle, metric, order, X, C):
    """list of every row: the canonical k = 1 of the row, as a query, over the centroids"""
    out = np.empty(X.shape[0], np.int64)
    for i in range(X.shape[0]):
        out[i] = oracle.topk_canonical(oracle.batch_flat(metric, X[i], C, order), 1)[0][0]
    return out


def probes(oracle, metric, order, q, C, nprobe):
    """the labels of the k = min(nprobe, nlist) search of the query over the centroids"""
    return oracle.topk_canonical(oracle.batch_flat(metric, q, C, order), min(nprobe, C.shape[0]))[0]


def probed_rows(lists, pr):
    """ascending rows whose list is one of pr"""
    return np.flatnonzero(np.isin(lists, pr))


def search(oracle, metric, order, Q, X, C, lists, k, nprobe, ids=None):
    """-> (labels [nq, k], dist [nq, k], rows scanned per query [nq])"""
    labels = np.empty((Q.shape[0], k), np.int64)
    dist = np.empty((Q.shape[0], k), F)
    scanned = np.empty(Q.shape[0], np.int64)
    for j in range(Q.shape[0]):
        rows = probed_rows(lists, probes(oracle, metric, order, Q[j], C, nprobe))
        scanned[j] = rows.size
        lab, d = oracle_topk_rows_parallel(oracle, metric, Q[j], X, k, nthreads=4, visible=rows, order=order)
        labels[j] = lab if ids is None else np.where(lab >= 0, ids[np.clip(lab, 0, None)], -1)
        dist[j] = d
    return labels, dist, scanned


def brute(oracle, metric, order, Q, X, k):
    labels = np.empty((Q.shape[0], k), np.int64)
    dist = np.empty((Q.shape[0], k), F)
    for j in range(Q.shape[0]):
        labels[j], dist[j] = oracle_topk_rows_parallel(oracle, metric, Q[j], X, k, nthreads=4, order=order)
    return labels, dist


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
def parity_case(n=3000, dim=16, nlist=16, nq=33, seed=1234):
    """standard-normal rows and queries; the centroids are nlist of the rows"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(F)
    Q = rng.standard_normal((nq, dim)).astype(F)
    C = X[np.sort(rng.permutation(n)[:nlist])].copy()
    return X, Q, C


def skew_case(n=50000, dim=8, seed=77):
    """centroids 0, +100, 0.5, -100 in every coordinate over standard-normal rows: list 0 takes about three quarters of them
    (more than the 32,768 keys beyond which no selection fits LDS), list 2 the rest, lists 1 and 3 stay empty.  Three queries sit
    near centroid 0 and two near centroid 2."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(F)
    C = np.stack([np.full(dim, v, F) for v in (0.0, 100.0, 0.5, -100.0)])
    Q = np.concatenate((rng.standard_normal((3, dim)).astype(F) * F(0.1) - F(0.5),
                        F(1.0) + rng.standard_normal((2, dim)).astype(F) * F(0.1)))
    return X, Q, C


def edge_case(counts, dim=8, seed=5, noise=0.01):
    """centroids 100 e_i; list i holds counts[i] rows (its centroid plus small noise), in shuffled insertion order; one query
    near each centroid"""
    rng = np.random.default_rng(seed)
    nlist = len(counts)
    C = (F(100.0) * np.eye(nlist, dim)).astype(F)
    owner = rng.permutation(np.repeat(np.arange(nlist), counts))
    X = (C[owner] + rng.standard_normal((owner.size, dim)).astype(F) * F(noise)).astype(F)
    Q = (C + rng.standard_normal((nlist, dim)).astype(F) * F(noise)).astype(F)
    return X, Q, C, owner
