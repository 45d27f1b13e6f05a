"""lb_gpu_ivf_train on the GPU -- ivf.train_coarse / train_coarse_device -- against tests/kmeans_oracle.py (any nlist) and,
where nlist <= 256, against lb_gpu_pq_train with M = 1: equal bytes of the centroids and equal iteration counts, no tolerance.

The E-step tile is 64 rows x 64 centroids x 64 elements, so the shapes are the smallest that leave it: more than one row
workgroup with a partial last one, several centroid tiles with a partial last one, whole chunks and a partial one, dims % 4 != 0
and dims = 1 (the generic form and the tail in chain 0), n == nlist, the limits dims = 8192 and nlist = 65,536."""
import functools

import numpy as np
import pytest

from tests import kmeans_oracle as ko
from tests.gpu_util import assert_same, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, CANCELLED = 1, 8


def _first_difference(got, want):
    bad = np.argwhere(np.ascontiguousarray(got, F).view(np.uint32) != np.ascontiguousarray(want, F).view(np.uint32))
    return f"{len(bad)} centroid words differ, first (c, j) {bad[:5].tolist()}"


def _same(got, want):
    assert got.shape == want.shape and got.dtype == F
    assert got.tobytes() == np.ascontiguousarray(want, F).tobytes(), _first_difference(got, want)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _clustered(n, dims, centres, seed):
    """rows around `centres` centres, a quarter of them midway between two: the drawn init rows leave some centres without a
    centroid and others with two, so assignments keep moving for a few iterations"""
    rng = np.random.default_rng(seed)
    Cn = rng.standard_normal((centres, dims))
    own = rng.integers(0, centres, n)
    other = rng.integers(0, centres, n)
    w = np.where(rng.random(n) < 0.25, rng.uniform(0.3, 0.7, n), 0.0)[:, None]
    return ((1 - w) * Cn[own] + w * Cn[other] + 0.5 * rng.standard_normal((n, dims))).astype(F)


@functools.lru_cache(maxsize=None)
def _oracle_case(name):
    """-> (rows, nlist, max_iter, seed, init rows or None, the oracle's centroids, its iterations): computed once, shared, frozen"""
    rows = None
    seed = 11
    if name == "clustered 1500x768x300":
        X, nlist = _clustered(1500, 768, 300, 1), 300
    elif name == "normal 700x100x257":
        X, nlist = np.random.default_rng(2).standard_normal((700, 100)).astype(F), 257
    elif name == "generic 600x7x300":
        X, nlist = np.random.default_rng(3).standard_normal((600, 7)).astype(F), 300
    elif name == "one dim, n == nlist 300x1x300":
        X, nlist = np.random.default_rng(4).standard_normal((300, 1)).astype(F), 300
    elif name == "few patterns 1000x24x300":
        X, nlist, seed = ko.few_pattern_rows(77, 1000, 24, 5), 300, 77
    elif name == "order sensitive 3000x4x260":
        X, nlist = ko.order_sensitive_rows(3000, 4), 260
    else:
        raise KeyError(name)
    max_iter = 3 if name == "clustered 1500x768x300" else 5  # (the oracle takes 1.5 s an iteration at that shape)
    want, iters = ko.train_kmeans(X, nlist, max_iter, rows, seed)
    return _frozen(X) + (nlist, max_iter, seed, rows, _frozen(want)[0], iters)


ORACLE_CASES = ["clustered 1500x768x300", "normal 700x100x257", "generic 600x7x300", "one dim, n == nlist 300x1x300",
                "few patterns 1000x24x300", "order sensitive 3000x4x260"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_train_coarse_is_train_kmeans(name):
    from longbow_amd import ivf
    gpu_or_skip()
    X, nlist, max_iter, seed, rows, want, want_iters = _oracle_case(name)
    print(name, "oracle iterations", want_iters)
    if name == "clustered 1500x768x300":
        assert want_iters >= 3
    if name == "normal 700x100x257":
        assert want_iters >= 3
    if name == "few patterns 1000x24x300":
        assert want_iters == 3 and np.unique(want, axis=0).shape[0] == 5
    got, iters = ivf.train_coarse(X, nlist, max_iter, seed, rows, return_iters=True)
    _same(got, want)
    assert iters == want_iters


@functools.lru_cache(maxsize=None)
def _repeated_init_case():
    """700 x 36 rows of which rows 10, 50, 400 and 650 are equal; init rows hold row 50 at positions 3, 200 and 290 (centroid
    tiles 0, 3 and 4)"""
    rng = np.random.default_rng(36)
    X = rng.standard_normal((700, 36)).astype(F)
    X[[10, 400, 650]] = X[50]
    others = np.setdiff1d(np.arange(700), [10, 50, 400, 650])
    rows = rng.permutation(others)[:300].astype(np.int64)
    rows[[3, 200, 290]] = 50
    return _frozen(X, rows)


def test_the_lowest_of_equal_centroids_takes_the_rows_across_tiles():
    from longbow_amd import ivf
    gpu_or_skip()
    X, rows = _repeated_init_case()
    seed, n, nlist = 21, 700, 300
    assign = ko.estep(X, X[rows])
    assert (assign[[10, 50, 400, 650]] == 3).all() and not np.isin(assign, [200, 290]).any()  # (what the oracle says)
    # iteration 0 alone: lists 200 and 290 are empty, so they are the drawn rows, and list 3 is the mean of its members in row order
    got, iters = ivf.train_coarse(X, nlist, 1, seed, rows, return_iters=True)
    assert iters == 1
    for c in (200, 290):
        _same(got[c], X[ko.draw(seed, 0, nlist + c) % n])
    members = np.flatnonzero(assign == 3)
    assert set((10, 50, 400, 650)) <= set(members.tolist())
    s = np.zeros(36, F)
    for r in members:
        s = s + X[r]
    _same(got[3], s / F(len(members)))
    _same(got, ko.train_kmeans(X, nlist, 1, rows, seed)[0])
    want, want_iters = ko.train_kmeans(X, nlist, 4, rows, seed)
    got, iters = ivf.train_coarse(X, nlist, 4, seed, rows, return_iters=True)
    _same(got, want)
    assert iters == want_iters


def _parent(X, nlist, max_iter, seed, rows):
    """lb_gpu_pq_train with M = 1 -> (centroids, iterations)"""
    from longbow_amd import pq
    blob, iters = pq.train(X, 1, nlist, max_iter, seed, None if rows is None else np.asarray(rows, np.int64).reshape(1, nlist))
    return np.frombuffer(blob[12:], "<f4").reshape(nlist, X.shape[1]), int(iters[0])


def _parent_case(name):
    rng = np.random.default_rng(len(name))
    if name == "1500x768x100":
        return rng.standard_normal((1500, 768)).astype(F), 100, 3, None
    if name == "300x8192x130":  # LB_MAX_DIM: 128 chunks, three centroid tiles, the last one partial
        return rng.standard_normal((300, 8192)).astype(F), 130, 2, rng.permutation(300)[:130]
    if name == "2000x32x256":
        return rng.standard_normal((2000, 32)).astype(F), 256, 3, None
    if name == "chain order":
        return ko.chain_order_rows(8), 256, 3, np.arange(256)
    if name == "sqrt tie":
        return ko.sqrt_tie_rows(), 2, 2, np.arange(2)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["1500x768x100", "300x8192x130", "2000x32x256", "chain order", "sqrt tie"])
def test_train_coarse_is_the_pq_trainer_with_one_subspace(name):
    from longbow_amd import ivf
    gpu_or_skip()
    X, nlist, max_iter, rows = _parent_case(name)
    want, want_iters = _parent(X, nlist, max_iter, 13, rows)
    got, iters = ivf.train_coarse(X, nlist, max_iter, 13, rows, return_iters=True)
    _same(got, want)
    assert iters == want_iters
    if name == "sqrt tie":  # the squared compare wins: in iteration 0 row 2 goes to centroid 1, and centroid 0 stays row 0
        first = ivf.train_coarse(X, 2, 1, 13, rows)
        _same(first, np.stack([X[0], (X[1] + X[2]) / F(2)]))
        _same(got, ko.train_kmeans(X, 2, max_iter, rows, 13)[0])


def test_closed_form_at_65536_lists():
    """row i = (i & 255, (i >> 8) & 255): every row equals exactly one of the first 65,536, so its list is i mod 65,536, the means
    are of equal small integers, nothing moves, and iteration 1 changes nothing"""
    from longbow_amd import ivf
    gpu_or_skip()
    i = np.arange(70000)
    X = np.stack([i & 255, (i >> 8) & 255], axis=1).astype(F)
    got, iters = ivf.train_coarse(X, 65536, 5, 0, np.arange(65536), return_iters=True)
    _same(got, X[:65536])
    assert iters == 2


def _raw(lib, X, nlist, max_iter, seed, rows, ctx=None):
    """the C call with pre-filled outputs -> (rc, centroids untouched, iters untouched)"""
    cent = np.full(nlist * X.shape[1] * 4, 0xAB, np.uint8)
    it = np.full(1, 0x5A5A5A5A, np.int32)
    r = None if rows is None else np.ascontiguousarray(rows, np.int64)
    rc = lib.lb_gpu_ivf_train(0, X.shape[1], nlist, X.shape[0], X.ctypes.data, max_iter, seed, r.ctypes.data if r is not None else None,
                              cent.ctypes.data, it.ctypes.data, ctx._h if ctx is not None else None)
    return rc, bool((cent == 0xAB).all()), bool(it[0] == 0x5A5A5A5A)


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("at", [(311, 5), (7, 0)])  # a row that is no init row, and init row 7 itself
def test_a_row_without_an_admissible_centroid_fails_the_call(value, at):
    from longbow_amd import _lib, ivf
    lib = gpu_or_skip()
    X = np.random.default_rng(8).standard_normal((600, 8)).astype(F)
    assert _raw(lib, X, 300, 3, 1, np.arange(300))[0] == 0
    X[at] = value
    assert _raw(lib, X, 300, 3, 1, np.arange(300)) == (INVALID, True, True)
    with pytest.raises(_lib.LongbowGPUError) as e:
        ivf.train_coarse(X, 300, 3, 1, np.arange(300))
    assert e.value.code == INVALID and type(e.value) is _lib.LongbowGPUError


def test_no_iterations_returns_the_init_rows():
    from longbow_amd import ivf
    gpu_or_skip()
    X = np.random.default_rng(9).standard_normal((700, 20)).astype(F)
    got, iters = ivf.train_coarse(X, 300, 0, 5, return_iters=True)
    _same(got, X[ko.init_rows(5, 0, 300, 700)])
    assert iters == 0
    rows = np.random.default_rng(10).integers(0, 700, 300)  # duplicates among them
    _same(ivf.train_coarse(X, 300, 0, 5, rows), X[rows])


def test_a_cancelled_token_stops_the_call():
    from longbow_amd import _lib, gpu, ivf
    lib = gpu_or_skip()
    X = np.random.default_rng(12).standard_normal((600, 8)).astype(F)
    c = gpu.Cancel()
    c.fire()
    assert _raw(lib, X, 300, 3, 1, None, c) == (CANCELLED, True, True)
    with pytest.raises(_lib.Canceled):
        ivf.train_coarse(X, 300, 3, 1, ctx=c)
    with pytest.raises(_lib.DeadlineExceeded):
        ivf.train_coarse(X, 300, 3, 1, ctx=gpu.Cancel(deadline_ms=0))
    _same(ivf.train_coarse(X, 300, 3, 1, ctx=gpu.Cancel(deadline_ms=600_000)), ivf.train_coarse(X, 300, 3, 1))


def test_device_entry_point():
    import torch
    from longbow_amd import ivf
    gpu_or_skip()
    X, nlist, max_iter, seed, rows, want, want_iters = _oracle_case("normal 700x100x257")
    dX = torch.from_numpy(np.array(X)).cuda()
    torch.cuda.synchronize()
    got, iters = ivf.train_coarse_device(700, dX.data_ptr(), 100, nlist, max_iter, seed, rows, return_iters=True)
    _same(got, want)
    _same(got, ivf.train_coarse(X, nlist, max_iter, seed, rows))
    assert iters == want_iters
    # a base that is not 16-byte aligned takes the generic form: rows 0.. of a buffer shifted by one float
    flat = torch.zeros(700 * 100 + 1, dtype=torch.float32, device="cuda")
    flat[1:] = dX.reshape(-1)
    torch.cuda.synchronize()
    _same(ivf.train_coarse_device(700, flat.data_ptr() + 4, 100, nlist, max_iter, seed, rows), want)
    given = np.arange(257)[::-1].copy()
    _same(ivf.train_coarse_device(700, dX.data_ptr(), 100, nlist, 0, seed, given), X[given])


def test_trained_lists_end_to_end():
    from longbow_amd import ivf, ivfpq, ivfsq8
    gpu_or_skip()
    rng = np.random.default_rng(16)
    X = _clustered(3000, 16, 300, 16)
    Q = rng.standard_normal((20, 16)).astype(F)
    cent = ivf.train_coarse(X, 300, 4, 2)
    assert cent.shape == (300, 16)
    h = ivf.IVFFlat(cent)
    h.add(X)
    assert int(h.list_sizes().sum()) == 3000
    flat = new_index(16)
    flat.Add(None, X)
    assert_same(*h.search(Q, 10, 300), *flat.SearchBatch(Q, 10), "every list probed")
    flat.Close()
    h.Close()
    idx = ivf.IVFFlatIndex(16, ivf.IVFFlatConfig(NClusters=300, NProbe=300), train_iters=4, seed=2)
    idx.AddBatch(np.arange(3000), X)
    idx.Build()
    _same(idx._h.centroids(), cent)
    assert idx.Size() == 3000 and int(idx.list_sizes().sum()) == 3000
    idx.Close()
    c2, blob = ivfpq.train(X, 300, 4, max_iter=2, seed=2, centroids=cent)
    assert c2 is cent and len(blob) == 12 + 4 * 256 * 4 * 4
    c3, blob3 = ivfpq.train(X, 300, 4, max_iter=2, seed=2, centroids=cent, residual=True)
    assert c3 is cent and blob3 != blob
    c4, mn, mx = ivfsq8.train(X, 300, centroids=cent)
    assert c4 is cent and mn.shape == mx.shape == (16,)
