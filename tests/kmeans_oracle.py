"""Numpy restatement of the PQ training semantics (include/longbow_gpu.h, "PQ training"): pq.TrainKMeans
(internal/pq/kmeans.go:64-151) per subspace with the documented counter-based draws.  TEST INFRASTRUCTURE ONLY.

E-step: oracle_np.l2sq_unroll4 sums, the first centroid strictly below the best so far (best starts at FLT_MAX).
M-step: one sequential f32 chain per (cluster, element) over the members in ascending row order -- vectorised over the
clusters, looped over the member rank -- then sum / float32(count).
"""
import struct

import numpy as np

from oracle import oracle_np

F = np.float32
MASK = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
FLT_MAX = np.finfo(F).max


def mix64(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, m, t):
    return mix64(mix64(seed + m) + (t + 1) * GAMMA)


def init_rows(seed, m, K, n):
    """the first K entries of a Fisher-Yates shuffle of [0, n): j = i + draw(seed, m, i) mod (n - i)"""
    moved = {}
    out = []
    for i in range(K):
        j = i + draw(seed, m, i) % (n - i)
        vi, vj = moved.get(i, i), moved.get(j, j)
        moved[j] = vi
        out.append(vj)
    return np.array(out, np.int64)


class NoCentroid(ValueError):
    """a row with no centroid below FLT_MAX: the reference indexes counts[-1] and panics"""


def estep(V, cent):
    """assignment of every row: first c with l2sq(v, cent_c) < best, best from FLT_MAX; -1 when there is none"""
    n = V.shape[0]
    best = np.full(n, FLT_MAX, F)
    assign = np.full(n, -1, np.int64)
    with np.errstate(all="ignore"):
        for c in range(cent.shape[0]):
            d = oracle_np.l2sq_unroll4(cent[c], V)
            lt = d < best
            best[lt] = d[lt]
            assign[lt] = c
    return assign


def mstep_sums(V, assign, K):
    """(sums [K, sub], counts [K]): sums[c] accumulated row by row in ascending row order"""
    order = np.argsort(assign, kind="stable")
    counts = np.bincount(assign, minlength=K)
    starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
    sums = np.zeros((K, V.shape[1]), F)
    live = np.arange(K)
    with np.errstate(all="ignore"):
        for r in range(int(counts.max())):
            live = live[counts[live] > r]
            sums[live] = sums[live] + V[order[starts[live] + r]]
    return sums, counts


def train_kmeans(V, K, max_iter, rows=None, seed=0, m=0):
    """TrainKMeans(V, n, sub, K, max_iter) -> (centroids [K, sub], iterations run)"""
    V = np.ascontiguousarray(V, F)
    n = V.shape[0]
    if n < K:
        raise ValueError("insufficient data for k-means: n < k")
    rows = init_rows(seed, m, K, n) if rows is None else np.asarray(rows, np.int64)
    cent = V[rows].copy()
    assign = np.full(n, -1, np.int64)
    iters = 0
    for it in range(max_iter):
        new = estep(V, cent)
        if (new < 0).any():
            raise NoCentroid(f"row {int(np.argmax(new < 0))} has no admissible centroid")
        changed = int((new != assign).sum())
        assign = new
        sums, counts = mstep_sums(V, assign, K)
        with np.errstate(all="ignore"):
            for c in range(K):
                if counts[c] > 0:
                    cent[c] = sums[c] / F(counts[c])
                else:
                    cent[c] = V[draw(seed, m, K + it * K + c) % n]
        iters = it + 1
        if it > 0 and changed < n // 1000 + 1:
            break
    return cent, iters


def train_pq(X, M, K, max_iter=20, seed=0, rows=None):
    """pq.(*PQEncoder).Train -> (codebooks [M, K, sub], iters [M]); rows: None or [M, K] init rows"""
    X = np.ascontiguousarray(X, F)
    n, dims = X.shape
    sub = dims // M
    cb = np.empty((M, K, sub), F)
    iters = np.zeros(M, np.int32)
    for m in range(M):
        cb[m], iters[m] = train_kmeans(X[:, m * sub:(m + 1) * sub], K, max_iter,
                                       None if rows is None else np.asarray(rows).reshape(M, K)[m], seed, m)
    return cb, iters


def blob(cb):
    """persistence.go:9-35"""
    M, K, sub = cb.shape
    return struct.pack("<III", M * sub, M, K) + np.ascontiguousarray(cb, "<f4").tobytes()


def order_sensitive_rows(n=3000, dims=4, seed=7):
    """rows spanning 1e-3 ... 1e4: a pairwise or a reversed-order f32 sum of a column differs from the sequential one"""
    rng = np.random.default_rng(seed)
    return (10.0 ** rng.uniform(-3.0, 4.0, (n, dims))).astype(F)


def few_pattern_rows(seed=77, n=1000, dims=24, patterns=5):
    """n rows, each one of `patterns` integer-valued patterns in [-8, 8]: every sum is exact, so the mean of a cluster that holds
    one pattern is that pattern, bit for bit.  With more centroids than patterns most clusters are empty after every iteration
    and are re-seeded from draw(seed, m, K + it*K + c); a re-seeded centroid ties with the holder of its pattern and the lower
    index takes the rows, so the result depends on every term of the draw."""
    return few_pattern_case(1, 1, seed, n, dims, patterns)[0]


def few_pattern_case(M, K, seed=77, n=1000, dims=24, patterns=5):
    """-> (few_pattern_rows(seed), init rows [M, K] as permutations from the same generator).  Train it with `seed` as well."""
    rng = np.random.default_rng(seed)
    P = rng.integers(-8, 9, (patterns, dims))
    X = P[rng.integers(0, patterns, n)].astype(F)
    rows = np.stack([rng.permutation(n)[:K] for _ in range(M)]).astype(np.int64)
    return X, rows


FEW_PATTERN_CASES = ((1, 16), (2, 16), (3, 40))  # (M, K) at 24 dimensions: sub = 24 (the generic E-step), 12 and 8 (templated)


def chain_order_rows(sub, K=256, levels=64, seed=9):
    """K rows that are permutations of one vector (the init rows: train with init rows 0 .. K-1), then `levels` rows a * (1, ..., 1).
    The differences of such a row to every centroid are one multiset in K orders, so its K sums are equal in exact arithmetic and
    a few ulp apart in f32: which centroid is the first strict minimum depends on the order in which the E-step adds -- which
    chain an element goes to, and how the chains combine."""
    rng = np.random.default_rng(seed)
    v = (rng.choice([-1.0, 1.0], sub) * 10.0 ** rng.uniform(-1.0, 1.0, sub)).astype(F)
    cent = np.stack([v[rng.permutation(sub)] for _ in range(K)])
    a = rng.uniform(-1.0, 1.0, levels).astype(F)
    return np.concatenate((cent, a[:, None] * np.ones((1, sub), F)))


def sqrt_tie_rows():
    """rows 0, 1 (the init rows) and 2 = the origin, sub = 2: row 2's sums to the two centroids are 1 + 3 ulp and 1 + 2 ulp,
    whose float32(sqrt(float64(.))) are equal.  The squared compare takes centroid 1, the sqrt compare (encode) centroid 0."""
    b3 = F(np.sqrt(3.0 * 2.0 ** -23))
    b2 = F(np.sqrt(2.0 * 2.0 ** -23))
    return np.array([[1.0, b3], [1.0, b2], [0.0, 0.0]], F)
