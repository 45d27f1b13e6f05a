"""The reference's DataTypeInt8 registry kernels (internal/simd/dispatch.go), restated twice:

- scalar transcriptions, line for line: euclideanInt8AVX2Kernel (simd_amd64.s), euclideanInt8Unrolled4x and dotInt8Unrolled4x
  (simd_baseline.go);
- a vectorised restatement for whole corpora, the oracle of the int8 index's tests.  Its integer sums come from float64 BLAS,
  exact here: every partial sum is an integer below 2^28.  The f32 steps that follow are applied as the reference applies
  them.

Reported distances follow the index: L2 the value, dot its negation; lists in ascending (distance, row) order.
"""
import numpy as np

F = np.float32


# ---- scalar transcriptions ------------------------------------------------------------------------------------------
def euclidean_int8_avx2(a, b):
    """euclideanInt8AVX2Kernel: int32 sum over 16-element blocks, VCVTDQ2PS, scalar f32 tail in order, VSQRTSS"""
    n = len(a)
    s = 0
    i = 0
    while n - i >= 16:
        for j in range(i, i + 16):
            d = int(a[j]) - int(b[j])
            s += d * d
        i += 16
    f = F(s)
    while i < n:
        d = int(a[i]) - int(b[i])
        f = F(f + F(d * d))
        i += 1
    return F(np.sqrt(np.float64(f)))


def euclidean_int8_unrolled4x(a, b):
    """euclideanInt8Unrolled4x: four f32 chains, tail in chain 0, float32(math.Sqrt(float64(s0 + s1 + s2 + s3)))"""
    s = [F(0)] * 4
    n = len(a)
    i = 0
    while i <= n - 4:
        for t in range(4):
            d = F(F(a[i + t]) - F(b[i + t]))
            s[t] = F(s[t] + F(d * d))
        i += 4
    while i < n:
        d = F(F(a[i]) - F(b[i]))
        s[0] = F(s[0] + F(d * d))
        i += 1
    tot = F(F(F(s[0] + s[1]) + s[2]) + s[3])
    return F(np.sqrt(np.float64(tot)))


def dot_int8_unrolled4x(a, b):
    """dotInt8Unrolled4x: four f32 chains, tail in chain 0, ((s0 + s1) + s2) + s3"""
    s = [F(0)] * 4
    n = len(a)
    i = 0
    while i <= n - 4:
        for t in range(4):
            s[t] = F(s[t] + F(F(a[i + t]) * F(b[i + t])))
        i += 4
    while i < n:
        s[0] = F(s[0] + F(F(a[i]) * F(b[i])))
        i += 1
    return F(F(F(s[0] + s[1]) + s[2]) + s[3])


# ---- vectorised restatement -----------------------------------------------------------------------------------------
def _isum(A, B):
    """exact integer A @ B.T of int8 blocks, as int64"""
    return np.rint(A.astype(np.float64) @ B.astype(np.float64).T).astype(np.int64)


def l2_values(Q, X):
    """(nq, n) f32: euclideanInt8AVX2Kernel of every (query, row) pair"""
    D = X.shape[1]
    m = 16 * (D // 16)
    Qm, Xm = Q[:, :m].astype(np.int64), X[:, :m].astype(np.int64)
    S = (Qm * Qm).sum(1)[:, None] + (Xm * Xm).sum(1)[None, :] - 2 * _isum(Q[:, :m], X[:, :m])
    f = S.astype(np.float64).astype(F)  # S < 2^31: exact in f64, one rounding to f32
    for i in range(m, D):
        d = Q[:, i].astype(np.int64)[:, None] - X[:, i].astype(np.int64)[None, :]
        f = (f + (d * d).astype(F)).astype(F)
    return np.sqrt(f.astype(np.float64)).astype(F)


def dot_chains(Q, X):
    """the four exact integer chains p0..p3 of dotInt8Unrolled4x, each (nq, n) int64"""
    D = X.shape[1]
    m4 = 4 * (D // 4)
    p = [_isum(Q[:, r:m4:4], X[:, r:m4:4]) for r in range(4)]
    if D > m4:
        p[0] = p[0] + _isum(Q[:, m4:], X[:, m4:])
    return p


def dot_values(Q, X):
    """(nq, n) f32: dotInt8Unrolled4x of every pair (chains exact: the index's dimension limit)"""
    p = [c.astype(np.float64).astype(F) for c in dot_chains(Q, X)]
    return ((p[0] + p[1]).astype(F) + p[2]).astype(F) + p[3]


def distances(metric, Q, X):
    """reported distances: L2 the value, dot (metric 2) its negation"""
    Q = np.atleast_2d(Q)
    if metric == 0:
        return l2_values(Q, X)
    if metric == 2:
        return (-dot_values(Q, X)).astype(F)
    raise ValueError("int8: L2 and dot only")


def topk(dist_row, k, rows=None):
    """canonical top-k of one query's distances: ascending (distance, row); -1 / FLT_MAX padding"""
    n = dist_row.shape[0]
    rows = np.arange(n) if rows is None else rows
    order = np.lexsort((rows, dist_row + F(0)))[:k]  # (+0: -0 and +0 are one key)
    lab = np.full(k, -1, np.int64)
    dist = np.full(k, np.finfo(F).max, F)
    lab[:len(order)] = rows[order]
    dist[:len(order)] = dist_row[order] + F(0)
    return lab, dist


def search(metric, Q, X, k, chunk=131072, ids=None, visible=None):
    """(labels, distances) of every query: the canonical top-k over X's rows (visible: the rows a mask leaves); the corpus is
    scored in chunks of rows so that a large one fits in memory"""
    Q = np.atleast_2d(Q)
    rows_all = np.arange(X.shape[0]) if visible is None else np.asarray(visible)
    best_d = np.empty((Q.shape[0], 0), F)
    best_r = np.empty((Q.shape[0], 0), np.int64)
    for c0 in range(0, len(rows_all), chunk):
        rr = rows_all[c0:c0 + chunk]
        d = distances(metric, Q, X[rr])
        cd = np.concatenate([best_d, d], 1)
        cr = np.concatenate([best_r, np.broadcast_to(rr, d.shape)], 1)
        kk = min(k, cd.shape[1])
        nd, nr = np.empty((Q.shape[0], kk), F), np.empty((Q.shape[0], kk), np.int64)
        for q in range(Q.shape[0]):
            o = np.lexsort((cr[q], cd[q] + F(0)))[:kk]
            nd[q], nr[q] = cd[q][o], cr[q][o]
        best_d, best_r = nd, nr
    lab = np.full((Q.shape[0], k), -1, np.int64)
    dist = np.full((Q.shape[0], k), np.finfo(F).max, F)
    kk = best_d.shape[1]
    lab[:, :kk] = best_r if ids is None else np.asarray(ids)[best_r]
    dist[:, :kk] = best_d + F(0)
    return lab, dist
