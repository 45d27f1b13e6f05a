"""The refine semantics of include/longbow_gpu.h (lb_gpu_index_refine) restated over what the suite already trusts: per query the
candidate set is the sorted distinct entries of its shortlist inside [0, ntotal); the distances are the C oracle's batch_flat over
those rows of X (on a float16 index: the rows widened to f32) and the result its topk_canonical, mapped back to rows and then to
ids.  That is tests/gpu_util.oracle_topk_rows_parallel with visible = the candidate set."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(F).max


def clean(rows, ntotal):
    """the candidate set of one shortlist, ascending"""
    r = np.asarray(rows, np.int64).reshape(-1)
    return np.unique(r[(r >= 0) & (r < ntotal)])


def refine_one(oracle, metric, q, X, rows, k, order, ids=None):
    """-> (labels [k], dist [k]), padded -1 / FLT_MAX"""
    S = clean(rows, X.shape[0])
    if S.size == 0:
        return np.full(k, -1, np.int64), np.full(k, FLT_MAX, F)
    d = oracle.batch_flat(metric, q, np.ascontiguousarray(X[S], F), order)
    oi, od, _ = oracle.topk_canonical(d, k)
    lab = np.where(oi >= 0, S[np.clip(oi, 0, S.size - 1)], -1).astype(np.int64)
    if ids is not None:
        lab = np.where(lab >= 0, np.asarray(ids, np.int64)[np.clip(lab, 0, None)], -1)
    return lab, od


def refine(oracle, metric, Q, X, rows, k, order, ids=None):
    """Q f32 [nq, dim], X [n, dim], rows int64 [nq, c] -> (labels [nq, k], dist [nq, k])"""
    Q = np.ascontiguousarray(Q, F)
    rows = np.asarray(rows, np.int64).reshape(Q.shape[0], -1)
    labels = np.empty((Q.shape[0], k), np.int64)
    dist = np.empty((Q.shape[0], k), F)
    for j in range(Q.shape[0]):
        labels[j], dist[j] = refine_one(oracle, metric, Q[j], X, rows[j], k, order, ids)
    return labels, dist
