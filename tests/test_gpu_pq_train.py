"""lb_gpu_pq_train on the GPU against tests/kmeans_oracle.py: the blob bytes and iters_out must equal the helper's exactly
(Lloyd's iteration is deterministic once the draws are fixed).  Shapes: every templated SubDim (1, 2, 4, 8, 12, 16, 32) and the
generic form (no 4-wide step: 3; tails of 1, 2, 3: 5, 6, 7; multiples of 4 without a template: 20, 24, 100), row counts around the
256-row workgroup, the 4096-row ordering chunk and the 64-row steps past a chunk, K from 1 to 256 on and off the 64-lane wave over
several chunks, clusters that stay empty in every iteration of every subspace, rows whose assignment is decided by the order of
the E-step's additions, skew, the stop rule, a caller's stream.  tests/test_gpu_coarse_train.py holds the coarse quantiser's
shapes (M = 1, sub = dims up to 8192)."""
import numpy as np
import pytest

from tests import kmeans_oracle as ko
from tests.gpu_util import gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32


def _rows(rng, M, K, n):
    return np.stack([rng.permutation(n)[:K] for _ in range(M)]).astype(np.int64)


def _check(X, M, K, max_iter, rows=None, seed=0):
    from longbow_amd import pq
    gpu_or_skip()
    cb, iters = ko.train_pq(X, M, K, max_iter, seed, rows)
    blob, git = pq.train(X, M, K, max_iter, seed, rows)
    assert git.tolist() == iters.tolist(), (git, iters)
    want = ko.blob(cb)
    if blob != want:
        got = np.frombuffer(blob[12:], "<f4").reshape(cb.shape)
        bad = np.argwhere(got.view(np.uint32) != cb.view(np.uint32))
        raise AssertionError(f"header {blob[:12] == want[:12]}; {len(bad)} centroid words differ, first (m, c, j) {bad[:5].tolist()}")
    return cb, iters


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("n", [256, 257, 300, 1000, 4099])
@pytest.mark.parametrize("sub", [1, 2, 4, 5, 8, 12, 16])
def test_k256_shapes(sub, n, M):
    rng = np.random.default_rng(1000 * sub + n + M)
    X = rng.standard_normal((n, M * sub)).astype(F)
    _check(X, M, 256, 3, _rows(rng, M, 256, n))


@pytest.mark.parametrize("M,n", [(1, 257), (1, 1000), (3, 257), (3, 1000)])
def test_k256_sub32(M, n):
    """km_estep_kernel<32>: the largest codebook in LDS, 32 KB"""
    rng = np.random.default_rng(32000 + n + M)
    X = rng.standard_normal((n, M * 32)).astype(F)
    _check(X, M, 256, 3, _rows(rng, M, 256, n))


def test_k100_sub32_two_chunks():
    rng = np.random.default_rng(32100)
    X = rng.standard_normal((4099, 32)).astype(F)
    _check(X, 1, 100, 3, _rows(rng, 1, 100, 4099))


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("sub", [3, 6, 7, 20, 24, 100])
def test_k256_generic_shapes(sub, M):
    """km_estep_generic_kernel: no main block (3), tails of 2 and 3 (6, 7), multiples of 4 without a template (20, 24, 100)"""
    rng = np.random.default_rng(7000 + 10 * sub + M)
    X = rng.standard_normal((300, M * sub)).astype(F)
    _check(X, M, 256, 3, _rows(rng, M, 256, 300))


@pytest.mark.parametrize("K,n,sub,M", [(65, 4500, 8, 1), (65, 4500, 8, 2), (100, 8193, 5, 1), (100, 8193, 5, 2), (200, 5000, 100, 1),
                                       (255, 4500, 20, 1)])
def test_k_off_the_wave_over_several_chunks(K, n, sub, M):
    """km_scan_kernel's idle lanes c >= K and km_scatter_kernel's eight-ballot rank with keys that stop short of a bit pattern"""
    rng = np.random.default_rng(K * 10000 + n + M)
    X = rng.standard_normal((n, M * sub)).astype(F)
    _check(X, M, K, 3, _rows(rng, M, K, n))


@pytest.mark.parametrize("n", [4096, 4097, 4159, 4160, 4161, 8192, 8193])
def test_chunk_and_wave_edges(n):
    """a full last chunk, one row past it, and the 64-row steps past a chunk where km_scatter_kernel leaves its step loop"""
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, 8)).astype(F)
    _check(X, 2, 16, 3, _rows(rng, 2, 16, n))


@pytest.mark.parametrize("seed", [77, 78])
@pytest.mark.parametrize("M,K,dims", [(M, K, 24) for M, K in ko.FEW_PATTERN_CASES] + [(1, 16, 20)])
def test_clusters_empty_in_every_iteration_of_every_subspace(M, K, dims, seed):
    """ko.few_pattern_case (tests/test_kmeans_semantics.py holds its properties): at least K - 5 clusters of every subspace are
    re-seeded in every iteration, and the result changes with the iteration, the seed and the subspace of the draw.  dims 24 at
    M = 1 and dims 20 go through the generic E-step, M = 2 and 3 through the templated 12 and 8."""
    X, rows = ko.few_pattern_case(M, K, seed)
    X = np.ascontiguousarray(X[:, :dims])
    for max_iter in (1, 2, 3, 6):
        _check(X, M, K, max_iter, rows, seed=seed)


def test_config4_geometry():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((600, 768)).astype(F)
    _check(X, 96, 256, 2, _rows(rng, 96, 256, 600))


@pytest.mark.parametrize("K", [1, 3, 16])
def test_small_k(K):
    rng = np.random.default_rng(K)
    X = rng.standard_normal((50, 12)).astype(F)
    _check(X, 3, K, 6, _rows(rng, 3, K, 50))
    _check(X[:, :5], 1, K, 6, _rows(rng, 1, K, 50))


def test_duplicate_init_rows_reseed_the_empty_cluster():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((300, 8)).astype(F)
    X[17] = X[5]  # duplicate rows, both among the init rows: the later copy's cluster is empty in iteration 0
    rows = np.array([[5, 17, 40, 41, 42, 43, 44, 45], [17, 5, 5, 60, 61, 62, 63, 64]], np.int64)
    cb, iters = _check(X, 2, 8, 4, rows, seed=77)
    # the helper took the re-seed path: after ONE iteration centroid 1 of subspace 0 is the copy of the drawn row
    cb1, _ = ko.train_pq(X, 2, 8, 1, 77, rows)
    assert cb1[0, 1].tobytes() == X[ko.draw(77, 0, 8 + 1) % 300, :4].tobytes()
    _check(X, 2, 8, 1, rows, seed=77)


def test_all_rows_equal():
    X = np.full((300, 8), 0.37, F)
    cb, iters = _check(X, 2, 4, 5, np.array([[0, 1, 2, 3], [9, 8, 7, 6]], np.int64), seed=3)
    assert np.isfinite(cb).all() and np.abs(cb - F(0.37)).max() < 1e-4


def test_order_sensitive_rows():
    X = ko.order_sensitive_rows()
    cb, _ = _check(X, 2, 2, 3, np.array([[0, 1], [5, 9]], np.int64))
    _check(X, 1, 1, 1, np.array([[0]], np.int64))
    _check(X, 2, 256, 2, _rows(np.random.default_rng(5), 2, 256, X.shape[0]))


def test_e_step_is_not_encode():
    X = ko.sqrt_tie_rows()
    cb, _ = _check(X, 1, 2, 1, np.array([[0, 1]], np.int64))
    assert cb[0, 0].tobytes() == X[0].tobytes()  # (the sqrt compare would have moved row 2 to centroid 0)


@pytest.mark.parametrize("sub", [7, 12, 32, 100])
def test_e_step_adds_in_the_reference_order(sub):
    """ko.chain_order_rows: every centroid is the same distance from a row in exact arithmetic, so the assignment is decided by
    which chain each element is added to and how the four chains combine (tests/test_kmeans_semantics.py: a sequential sum, the
    last 4-wide step in chain 0 or a pairwise total move at least a quarter of the rows)"""
    X = ko.chain_order_rows(sub)
    _check(X, 1, 256, 2, np.arange(256, dtype=np.int64)[None])
    _check(np.concatenate((X[:, ::-1], X), axis=1), 2, 256, 2, np.stack((np.arange(256), np.arange(256))).astype(np.int64))


def test_skew_across_workgroups_and_chunks():
    """one cluster of more than 4096 members (its members span every 4096-row chunk and 256-row workgroup), several of one"""
    rng = np.random.default_rng(21)
    n, K = 20000, 64
    X = rng.standard_normal((n, 32)).astype(F)
    big = rng.permutation(n)[:7000]
    X[big] = F(40.0) + rng.standard_normal((7000, 32)).astype(F) * F(0.01)
    lone = np.array([3, 4097, 8191, 12288, 19999])
    lone = lone[~np.isin(lone, big)]
    X[lone] = (F(-300.0) * (1 + np.arange(lone.size, dtype=F)))[:, None]
    rest = np.setdiff1d(np.arange(n), np.concatenate((big, lone)))
    rows = np.stack([np.concatenate(([big[m]], lone, rng.permutation(rest)[:K - 1 - lone.size])) for m in range(4)]).astype(np.int64)
    cb, iters = _check(X, 4, K, 5, rows)
    as0 = ko.estep(X[:, :8], cb[0])
    cnt = np.bincount(as0, minlength=K)
    assert cnt.max() > 4096 and (cnt == 1).sum() >= lone.size >= 3


def test_stop_rule():
    rng = np.random.default_rng(31)
    centres = rng.standard_normal((4, 8)).astype(F) * F(50)
    X = (centres[np.arange(2000) % 4] + rng.standard_normal((2000, 8)).astype(F) * F(0.1)).astype(F)
    _, iters = _check(X, 2, 4, 20, np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.int64))
    assert iters.tolist() == [2, 2]  # separated clusters: nothing moves in the second iteration
    U = rng.random((5000, 8), dtype=F)
    _, iters = _check(U, 2, 256, 3, _rows(rng, 2, 256, 5000))
    assert iters.tolist() == [3, 3]  # uniform noise runs all of max_iter
    # subspaces stop independently: subspace 0 separated, subspace 1 noise
    Y = np.concatenate((X[:, :4], U[:2000, :4]), axis=1)
    _, iters = _check(Y, 2, 4, 6, np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.int64))
    assert iters[0] == 2 and iters[1] > 2
    for mi in (0, 1):
        cb, iters = _check(U[:700], 2, 256, mi, _rows(rng, 2, 256, 700))
        assert iters.tolist() == [mi, mi]


@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
def test_drawn_init_rows(seed):
    rng = np.random.default_rng(41)
    X = rng.standard_normal((257, 12)).astype(F)
    _check(X, 3, 256, 2, None, seed)
    _check(X[:256], 3, 256, 0, None, seed)  # n = K: max_iter 0 returns the drawn rows, a permutation of all of them
    _check(rng.standard_normal((3000, 8)).astype(F), 2, 16, 4, None, seed)


def test_host_and_device_entry_points_agree():
    import torch
    from longbow_amd import pq
    gpu_or_skip()
    rng = np.random.default_rng(51)
    X = rng.standard_normal((1500, 24)).astype(F)
    rows = _rows(rng, 3, 256, 1500)
    dX = torch.from_numpy(X).cuda()
    torch.cuda.synchronize()
    for r in (rows, None):
        blob, iters = pq.train(X, 3, 256, 3, 9, r)
        dblob, diters = pq.train_device(1500, dX.data_ptr(), 24, 3, 256, 3, 9, r)
        assert blob == dblob and iters.tolist() == diters.tolist()
    cb, iters = ko.train_pq(X, 3, 256, 3, 9, rows)
    assert pq.train_device(1500, dX.data_ptr(), 24, 3, 256, 3, 9, rows)[0] == ko.blob(cb)


def test_rows_without_an_admissible_centroid_are_refused():
    lib = gpu_or_skip()
    rng = np.random.default_rng(61)

    def run(X, M, K, rows):
        blob = np.full(12 + M * K * (X.shape[1] // M) * 4, 0xAB, np.uint8)
        iters = np.zeros(M, np.int32)
        rc = lib.lb_gpu_pq_train(0, X.shape[1], M, K, X.shape[0], X.ctypes.data, 3, 0, rows.ctypes.data, blob.ctypes.data, blob.size,
                                 iters.ctypes.data, None)
        return rc, blob

    X = rng.standard_normal((600, 8)).astype(F)
    X[311, 5] = np.nan
    rows = np.arange(16, dtype=np.int64).reshape(2, 8)
    rc, blob = run(X, 2, 8, rows)
    assert rc == 1 and (blob == 0xAB).all()
    W = np.full((300, 4), -3e38, F)
    W[299] = 3e38  # every difference overflows: the sum is +inf, not below FLT_MAX
    rc, blob = run(W, 1, 2, np.array([[0, 1]], np.int64))
    assert rc == 1 and (blob == 0xAB).all()
    X[311, 5] = 0.0
    rc, blob = run(X, 2, 8, rows)
    assert rc == 0 and blob.tobytes() == ko.blob(ko.train_pq(X, 2, 8, 3, 0, rows)[0])


def test_rows_without_an_admissible_centroid_are_refused_by_the_generic_form():
    lib = gpu_or_skip()
    rng = np.random.default_rng(62)
    X = rng.standard_normal((600, 100)).astype(F)
    X[311, 97] = np.nan
    rows = np.arange(8, dtype=np.int64).reshape(1, 8)

    def run():
        blob = np.full(12 + 8 * 100 * 4, 0xAB, np.uint8)
        iters = np.zeros(1, np.int32)
        rc = lib.lb_gpu_pq_train(0, 100, 1, 8, 600, X.ctypes.data, 3, 0, rows.ctypes.data, blob.ctypes.data, blob.size, iters.ctypes.data,
                                 None)
        return rc, blob

    rc, blob = run()
    assert rc == 1 and (blob == 0xAB).all()
    X[311, 97] = 0.0
    rc, blob = run()
    assert rc == 0 and blob.tobytes() == ko.blob(ko.train_pq(X, 1, 8, 3, 0, rows)[0])


def test_a_callers_stream():
    """the rows' upload is enqueued on the caller's stream and nothing waits for it before the call: the training runs behind it"""
    import torch
    from longbow_amd import pq
    gpu_or_skip()
    rng = np.random.default_rng(52)
    n = 100000  # (a 9.6 MB upload: still in flight when the call is made)
    X = rng.standard_normal((n, 24)).astype(F)
    rows = _rows(rng, 3, 16, n)
    want, wit = pq.train(X, 3, 16, 2, 9, rows)
    cb, iters = ko.train_pq(X, 3, 16, 2, 9, rows)
    assert want == ko.blob(cb) and wit.tolist() == iters.tolist()
    host = torch.from_numpy(X).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dX = host.to("cuda", non_blocking=True)
        blob, git = pq.train_device(n, dX.data_ptr(), 24, 3, 16, 2, 9, rows, stream=s.cuda_stream)
    assert blob == want and git.tolist() == wit.tolist()
    torch.cuda.synchronize()


def test_a_cancelled_token_stops_the_call():
    from longbow_amd import _lib, gpu, pq
    gpu_or_skip()
    X = np.random.default_rng(71).standard_normal((400, 8)).astype(F)
    c = gpu.Cancel()
    c.fire()
    with pytest.raises(_lib.Canceled):
        pq.train(X, 2, 16, 5, ctx=c)
    with pytest.raises(_lib.DeadlineExceeded):
        pq.train(X, 2, 16, 5, ctx=gpu.Cancel(deadline_ms=0))
    blob, iters = pq.train(X, 2, 16, 5, ctx=gpu.Cancel(deadline_ms=600_000))
    assert blob == pq.train(X, 2, 16, 5)[0]


def test_train_encode_search_end_to_end():
    from longbow_amd import pq
    gpu_or_skip()
    rng = np.random.default_rng(81)
    n, dims, M = 3000, 32, 4
    centres = rng.standard_normal((40, dims)).astype(F) * F(3)
    X = (centres[rng.integers(0, 40, n)] + rng.standard_normal((n, dims)).astype(F) * F(0.3)).astype(F)
    rows = _rows(rng, M, 256, n)

    def mse(enc):
        codes = enc.Encode(X)
        d = X - enc.Decode(codes)
        return codes, float((d.astype(np.float64) ** 2).sum(axis=1).mean())

    enc = pq.PQEncoder.Train(X, M, init_rows=rows)
    assert (enc.M, enc.Dims, enc.K) == (M, dims, 256)
    codes, trained = mse(enc)
    enc.add_codes(codes)
    lab, dist = enc.Search(X[:3], 5)
    assert lab.shape == (3, 5) and (lab >= 0).all() and np.isfinite(dist).all() and (np.diff(dist, axis=1) >= 0).all()
    enc.Close()
    raw = pq.PQEncoder(pq.train(X, M, 256, 0, init_rows=rows)[0])  # the untrained init rows
    _, untrained = mse(raw)
    raw.Close()
    assert trained < untrained, (trained, untrained)
