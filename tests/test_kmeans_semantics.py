"""The PQ training semantics (include/longbow_gpu.h, "PQ training") on the CPU: tests/kmeans_oracle.py against a plain scalar
Lloyd loop, the properties the GPU kernels must keep (row order of the M-step, squared compare of the E-step, the draws),
and the reference's own TrainKMeans tests (internal/pq/kmeans_test.go) as properties -- its data is unseeded random."""
import numpy as np
import pytest

from oracle import oracle_np
from tests import kmeans_oracle as ko

F = np.float32


def _l2sq_scalar(a, b):
    """simd.L2Squared, one f32 operation at a time"""
    s = [F(0), F(0), F(0), F(0)]
    n = len(a)
    i = 0
    while i <= n - 4:
        for u in range(4):
            d = F(a[i + u] - b[i + u])
            s[u] = F(s[u] + F(d * d))
        i += 4
    while i < n:
        d = F(a[i] - b[i])
        s[0] = F(s[0] + F(d * d))
        i += 1
    return F(F(F(s[0] + s[1]) + s[2]) + s[3])


def _lloyd_scalar(V, K, max_iter, rows, seed, m):
    """kmeans.go:64-151 line by line (assignments start at -1, the draws as documented)"""
    n, dim = V.shape
    cent = [[F(x) for x in V[r]] for r in rows]
    assign = [-1] * n
    iters = 0
    for it in range(max_iter):
        sums = [[F(0)] * dim for _ in range(K)]
        counts = [0] * K
        changed = 0
        for i in range(n):
            best, bc = np.finfo(F).max, -1
            for c in range(K):
                d = _l2sq_scalar(V[i], cent[c])
                if d < best:
                    best, bc = d, c
            if assign[i] != bc:
                changed += 1
                assign[i] = bc
            counts[bc] += 1
            for j in range(dim):
                sums[bc][j] = F(sums[bc][j] + V[i][j])
        for c in range(K):
            if counts[c] > 0:
                cent[c] = [F(sums[c][j] / F(counts[c])) for j in range(dim)]
            else:
                cent[c] = [F(x) for x in V[ko.draw(seed, m, K + it * K + c) % n]]
        iters = it + 1
        if it > 0 and changed < n // 1000 + 1:
            break
    return np.array(cent, F), iters


@pytest.mark.parametrize("n,K,sub", [(40, 5, 3), (64, 8, 8)])
def test_helper_equals_a_scalar_lloyd_loop(n, K, sub):
    rng = np.random.default_rng(n)
    V = rng.standard_normal((n, sub)).astype(F)
    rows = ko.init_rows(3, 1, K, n)
    want, wit = _lloyd_scalar(V, K, 20, rows, 3, 1)
    got, git = ko.train_kmeans(V, K, 20, seed=3, m=1)
    assert git == wit and got.tobytes() == want.tobytes()
    # duplicate init rows: the second copy's cluster stays empty and is re-seeded by the draw
    rows2 = rows.copy()
    rows2[1] = rows2[0]
    want, wit = _lloyd_scalar(V, K, 4, rows2, 9, 0)
    got, git = ko.train_kmeans(V, K, 4, rows=rows2, seed=9, m=0)
    assert git == wit and got.tobytes() == want.tobytes()


def test_the_row_order_of_the_m_step_matters():
    V = ko.order_sensitive_rows()
    assert V.min() >= 1e-3 * 0.99 and V.max() <= 1e4 * 1.01 and V.max() / V.min() > 1e6
    n = V.shape[0]
    cent, iters = ko.train_kmeans(V[:, :2], 1, 1, rows=[0])
    seq = np.zeros(2, F)
    rev = np.zeros(2, F)
    for i in range(n):
        seq = seq + V[i, :2]
        rev = rev + V[n - 1 - i, :2]
    pair = V[:, :2].copy()  # a tree: neighbours first
    while pair.shape[0] > 1:
        if pair.shape[0] % 2:
            pair = np.concatenate((pair, np.zeros((1, 2), F)))
        pair = pair[0::2] + pair[1::2]
    pair = pair[0]
    assert iters == 1 and cent[0].tobytes() == (seq / F(n)).tobytes()
    assert (rev / F(n)).tobytes() != cent[0].tobytes()
    assert (pair / F(n)).tobytes() != cent[0].tobytes()


def test_e_step_compares_sums_where_encode_compares_square_roots():
    V = ko.sqrt_tie_rows()
    cent = V[:2]
    s = oracle_np.l2sq_unroll4(V[2], cent)
    r = oracle_np.euclidean(V[2], cent, order="unroll4")
    assert s[1] < s[0] and r[0] == r[1]
    assert ko.estep(V, cent).tolist() == [0, 1, 1]  # the later centroid: its sum is strictly smaller
    enc = 0
    for c in range(1, 2):  # encode (simd.FindNearestCentroid): first strict minimum of the rounded square roots
        if r[c] < r[enc]:
            enc = c
    assert enc == 0
    got, _ = ko.train_kmeans(V, 2, 1, rows=[0, 1])
    assert got[0].tobytes() == V[0].tobytes()
    assert got[1].tobytes() == ((V[1] + V[2]) / F(2)).tobytes()


@pytest.mark.parametrize("extra", [0, 1])
def test_init_draws_are_distinct_and_in_range(extra):
    K = 256
    n = K + extra
    for seed in (0, 1, 2 ** 63 + 5):
        for m in (0, 7):
            rows = ko.init_rows(seed, m, K, n)
            assert rows.min() >= 0 and rows.max() < n and len(set(rows.tolist())) == K
    assert not np.array_equal(ko.init_rows(0, 0, K, n), ko.init_rows(0, 1, K, n)) or n == 1
    assert ko.mix64(0) == 0 and ko.draw(0, 0, 0) == ko.mix64(ko.mix64(0) + ko.GAMMA)
    assert ko.mix64(ko.GAMMA) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0


def test_three_separated_clusters_are_recovered():
    """TestTrainKMeans_Basic"""
    rng = np.random.default_rng(1)
    centres = np.array([[1.0] * 16, [-1.0] * 16, [0.0] * 16], F)
    V = (centres[np.arange(300) // 100] + (rng.random((300, 16), dtype=F) - F(0.5)) * F(0.1)).astype(F)
    for seed in range(4):
        cent, iters = ko.train_kmeans(V, 3, 20, seed=seed)
        match = sum(any(((c - o) ** 2).sum() < 1.0 for o in centres) for c in cent)
        assert cent.shape == (3, 16) and match >= 2 and 1 <= iters <= 20
    cent, iters = ko.train_kmeans(V, 3, 20, rows=[0, 100, 200])
    assert iters == 2  # nothing changes in the second iteration: stopped by changed < n/1000 + 1
    assert all(min(((c - o) ** 2).sum() for o in centres) < 0.01 for c in cent)


def test_fewer_rows_than_centroids_is_an_error():
    """TestTrainKMeans_EmptyCluster"""
    with pytest.raises(ValueError, match="insufficient data for k-means: n < k"):
        ko.train_kmeans(np.random.default_rng(0).random((5, 8), dtype=F), 10, 5)


def test_one_iteration_and_zero():
    """TestTrainKMeans_SingleIteration"""
    V = np.random.default_rng(456).random((100, 8), dtype=F)
    cent, iters = ko.train_kmeans(V, 4, 1)
    assert cent.shape == (4, 8) and iters == 1
    cent0, iters0 = ko.train_kmeans(V, 4, 0)
    assert iters0 == 0 and cent0.tobytes() == V[ko.init_rows(0, 0, 4, 100)].tobytes()


def test_centroids_are_finite():
    """TestTrainKMeans_CentroidCount"""
    V = np.random.default_rng(999).random((1000, 32), dtype=F)
    cent, iters = ko.train_kmeans(V, 16, 5)
    assert cent.shape == (16, 32) and np.isfinite(cent).all() and np.abs(cent).max() < 1e10 and iters == 5


def test_a_row_without_an_admissible_centroid_is_refused():
    V = np.random.default_rng(2).random((20, 4), dtype=F)
    V[7, 1] = np.nan
    with pytest.raises(ko.NoCentroid):
        ko.train_kmeans(V, 3, 2, rows=[0, 1, 2])
    W = np.full((5, 2), -3e38, F)
    W[4] = 3e38
    with pytest.raises(ko.NoCentroid):
        ko.train_kmeans(W, 2, 2, rows=[0, 1])


# ---- what tests/test_gpu_pq_train.py and tests/test_gpu_coarse_train.py rely on in their inputs ---------------------------------
@pytest.mark.parametrize("sub", [3, 6, 7, 20])
def test_helper_equals_a_scalar_lloyd_loop_at_the_generic_shapes(sub):
    """no 4-wide step (3), a 2- and a 3-element tail (6, 7), five 4-wide steps and no tail (20)"""
    rng = np.random.default_rng(100 + sub)
    V = rng.standard_normal((40, sub)).astype(F)
    rows = ko.init_rows(5, 0, 3, 40)
    want, wit = _lloyd_scalar(V, 3, 2, rows, 5, 0)
    got, git = ko.train_kmeans(V, 3, 2, seed=5)
    assert git == wit == 2 and got.tobytes() == want.tobytes()


# iterations run at max_iter = 6, per subspace, of ko.few_pattern_case(M, K, seed) trained with the same seed
FEW_PATTERN_ITERS = {(1, 16, 77): [3], (2, 16, 77): [3, 3], (3, 40, 77): [2, 3, 3],
                     (1, 16, 78): [4], (2, 16, 78): [4, 4], (3, 40, 78): [4, 3, 4]}


@pytest.mark.parametrize("seed", [77, 78])
@pytest.mark.parametrize("M,K", ko.FEW_PATTERN_CASES)
def test_few_pattern_rows_keep_clusters_empty_in_every_iteration(M, K, seed):
    X, rows = ko.few_pattern_case(M, K, seed)
    assert X.shape == (1000, 24) and X.tobytes() == ko.few_pattern_rows(seed).tobytes()
    assert np.unique(X, axis=0).shape[0] == 5 and (X == np.rint(X)).all() and np.abs(X).max() <= 8
    sub = 24 // M
    by_iter = [ko.train_pq(X, M, K, mi, seed, rows) for mi in range(7)]
    assert by_iter[6][1].tolist() == FEW_PATTERN_ITERS[M, K, seed]
    for m in range(M):
        V = X[:, m * sub:(m + 1) * sub]
        for it in range(by_iter[6][1][m]):  # the E-step of iteration `it` sees the centroids of max_iter = it
            assert by_iter[it][1][m] == it
            counts = np.bincount(ko.estep(V, by_iter[it][0][m]), minlength=K)
            assert (counts == 0).sum() >= K - 5 >= 1, (m, it, counts)
        # exact sums: a centroid is a pattern, and several centroids are the same pattern
        final = by_iter[6][0][m]
        assert {c.tobytes() for c in final} <= {v.tobytes() for v in V}
        assert np.unique(final, axis=0).shape[0] < K
        # the draw's `it` term, its seed and its m are all observable
        assert by_iter[1][0][m].tobytes() != by_iter[2][0][m].tobytes()
        assert ko.train_kmeans(V, K, 6, rows[m], seed + 1, m)[0].tobytes() != final.tobytes()
        assert ko.train_kmeans(V, K, 6, rows[m], seed, m + 1)[0].tobytes() != final.tobytes()
    if M >= 2:  # subspaces with equal rows and equal init rows differ by the m of their draws alone
        V2 = np.concatenate((X[:, :sub], X[:, :sub]), axis=1)
        for mi in (1, 2, 6):
            cb, _ = ko.train_pq(V2, 2, K, mi, seed, np.stack((rows[0], rows[0])))
            assert cb[0].tobytes() == by_iter[mi][0][0].tobytes() and cb[1].tobytes() != cb[0].tobytes()


def test_few_pattern_rows_through_the_generic_width():
    """the first 20 columns (five 4-wide steps, no template) keep the five patterns apart and the clusters empty"""
    for seed in (77, 78):
        X, rows = ko.few_pattern_case(1, 16, seed)
        V = X[:, :20]
        assert np.unique(V, axis=0).shape[0] == 5
        one, two = ko.train_kmeans(V, 16, 1, rows[0], seed)[0], ko.train_kmeans(V, 16, 2, rows[0], seed)[0]
        assert one.tobytes() != two.tobytes()
        assert (np.bincount(ko.estep(V, one), minlength=16) == 0).sum() >= 11


def _unroll4_variant(q, X, last4_in_chain0=False, pairwise_total=False):
    """l2sq_unroll4 with one thing changed: the last full 4-wide step added to chain 0, or the chains combined as a tree"""
    n = X.shape[1]
    main = (n & ~3) - (4 if last4_in_chain0 else 0)
    acc = [np.zeros(X.shape[0], F) for _ in range(4)]
    for i in range(n):
        d = q[i] - X[:, i]
        u = i % 4 if i < main else 0
        acc[u] = acc[u] + d * d
    return (acc[0] + acc[1]) + (acc[2] + acc[3]) if pairwise_total else ((acc[0] + acc[1]) + acc[2]) + acc[3]


@pytest.mark.parametrize("sub", [7, 12, 32, 100])
def test_chain_order_rows_tell_the_summation_orders_apart(sub):
    X = ko.chain_order_rows(sub)
    cent, level = X[:256], X[256:]
    assert X.shape == (320, sub) and all(sorted(c.tolist()) == sorted(cent[0].tolist()) for c in cent)
    assert all(np.array_equal(_unroll4_variant(c, level), oracle_np.l2sq_unroll4(c, level)) for c in cent[:8])
    want = ko.estep(level, cent)
    assert np.unique(want).size >= 16  # no one centroid is the minimum of every row

    def estep(l2sq):
        best, assign = np.full(64, ko.FLT_MAX, F), np.full(64, -1)
        for c in range(256):
            d = l2sq(cent[c], level)
            lt = d < best
            best[lt], assign[lt] = d[lt], c
        return assign

    assert np.array_equal(estep(oracle_np.l2sq_unroll4), want)
    for other in (oracle_np.l2sq_seq, lambda q, V: _unroll4_variant(q, V, last4_in_chain0=True),
                  lambda q, V: _unroll4_variant(q, V, pairwise_total=True)):
        assert (estep(other) != want).sum() >= 16  # a quarter of the rows; 38 to 64 of them do
