"""lb_gpu_ivf_* on the GPU against tests/ivf_oracle.py (the semantics restated over the C oracle's batch_flat and
topk_canonical): labels and distances must be equal, bit for bit.  The shapes are the smallest at which the kernels can still go
wrong: lists around the 128-row tile, a list that needs the tile stride loop, a workgroup that walks several tiles of several
chunks, selections within LDS and beyond it, the staged scan
with one chunk, a partial last chunk and twelve, the one-lane-per-row form, more queries than a batch."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import ivf_oracle as io
from tests import kmeans_oracle as ko
from tests.gpu_util import assert_same, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED, CANCELLED = 1, 6, 8
LB_MAX_K = 2048
LDS_KEYS = 16384  # IVF_SELECT_LDS_KEYS: a query with more scanned rows is selected from global memory


def _handle(X, C_, metric=0, order=0, ids=None):
    from longbow_amd import ivf
    gpu_or_skip()
    h = ivf.IVFFlat(C_, metric, order)
    if X.shape[0]:
        h.add(X, ids)
    return h


def _check_search(oracle, h, metric, order, Q, X, C_, lists, k, nprobe, ids=None, ctx=""):
    ol, od, scanned = io.search(oracle, metric, order, Q, X, C_, lists, k, nprobe, ids=ids)
    lab, dist = h.search(Q, k, nprobe)
    assert_same(lab, dist, ol, od, ctx)
    st = h.last_search_stats()
    assert st[0] == Q.shape[0] and st[1] == int(scanned.sum()) and st[2] == int(scanned.max()), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= LDS_KEYS).sum()), (st, ctx)
    return scanned


@pytest.fixture(scope="module")
def parity(oracle):
    """the shape of case 1 with its oracle lists at metric 0, order 0 (shared by the adds, batches and mirror cases)"""
    X, Q, C_ = io.parity_case()
    return X, Q, C_, io.assign(oracle, 0, 0, X, C_)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_parity_grid(oracle, metric, order):
    X, Q, C_ = io.parity_case()
    lists = io.assign(oracle, metric, order, X, C_)
    h = _handle(X, C_, metric, order)
    assert h.ntotal == X.shape[0] and (h.nlist, h.dims) == C_.shape
    assert np.array_equal(h.assignments(), lists)
    assert np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    assert np.array_equal(h.centroids(), C_)
    for nprobe in (1, 3, 16):
        _check_search(oracle, h, metric, order, Q, X, C_, lists, 10, nprobe, ctx=f"metric {metric} order {order} nprobe {nprobe}")
    h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_every_list_probed_equals_the_flat_index(metric):
    X, Q, C_ = io.parity_case()
    for order in (0, 1):
        h = _handle(X, C_, metric, order)
        flat = new_index(X.shape[1], metric, order)
        flat.Add(None, X)
        fl, fd = flat.SearchBatch(Q, 10)
        for nprobe in (16, 21):
            lab, dist = h.search(Q, 10, nprobe)
            assert_same(lab, dist, fl, fd, f"metric {metric} order {order} nprobe {nprobe}")
            assert h.last_search_stats()[1] == Q.shape[0] * X.shape[0]
        flat.Close()
        h.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3, 5, 8, 100, 768])
def test_dimensions(oracle, dim):
    """1, 3, 5: the one-lane-per-row form; 8: one chunk; 100: a partial last chunk; 768: twelve chunks"""
    n, nlist, nprobe, k, nq = (3000, 16, 4, 100, 3) if dim == 768 else (1000, 7, 2, 10, 9)
    X, Q, C_ = io.parity_case(n, dim, nlist, nq, seed=dim)
    for metric, order in ((0, 0), (1, 1), (2, 1), (0, 1)):
        lists = io.assign(oracle, metric, order, X, C_)
        h = _handle(X, C_, metric, order)
        assert np.array_equal(h.assignments(), lists)
        _check_search(oracle, h, metric, order, Q, X, C_, lists, k, nprobe, ctx=f"dim {dim} metric {metric} order {order}")
        h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_list_length_edges(oracle):
    counts = (0, 1, 127, 128, 129, 257)
    X, Q, C_, owner = io.edge_case(counts)
    h = _handle(X, C_)
    assert np.array_equal(h.assignments(), owner) and h.list_sizes().tolist() == list(counts)
    for nprobe in (1, 2):
        for k in (10, 200):
            _check_search(oracle, h, 0, 0, Q, X, C_, owner, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
    lab, dist = h.search(Q, 10, 1)
    assert (lab[0] == -1).all() and (dist[0] == io.FLT_MAX).all()  # an empty probed list: all padding
    assert lab[1, 0] == np.flatnonzero(owner == 1)[0] and (lab[1, 1:] == -1).all() and (dist[1, 1:] == io.FLT_MAX).all()
    h.Close()


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("metric", [0, 1])
def test_one_workgroup_walks_several_tiles_and_chunks(oracle, metric, order):
    """1024 queries x 4 probes = 4,096 pairs, so the scan's grid has one workgroup per (query, list): it walks the three or more
    128-row tiles of the longest list, the last one partial, in three chunks each (136 dims: 64 + 64 + 8), and the pipeline wraps
    from a tile's last chunk to the next tile's first"""
    TILE, CHUNK, GRID = 128, 64, 4096
    nq, nprobe, dim = 1024, 4, 136
    X, Q, C_ = io.parity_case(2400, dim, 8, nq, seed=136)
    lists = io.assign(oracle, metric, order, X, C_)
    big = int(np.bincount(lists, minlength=8).max())
    assert max(1, -(-GRID // (nq * nprobe))) == 1  # grid.x
    assert big > 2 * TILE and big % TILE != 0, big
    assert -(-dim // CHUNK) >= 2 and dim % CHUNK != 0
    h = _handle(X, C_, metric, order)
    assert np.array_equal(h.assignments(), lists)
    _check_search(oracle, h, metric, order, Q, X, C_, lists, 10, nprobe, ctx=f"several tiles and chunks, metric {metric} order {order}")
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skew(oracle):
    X, Q, C_ = io.skew_case()
    return X, Q, C_, io.assign(oracle, 0, 0, X, C_)


def test_skew_and_the_long_selection(oracle, skew):
    X, Q, C_, lists = skew
    h = _handle(X, C_)
    assert np.array_equal(h.assignments(), lists)
    from_lds = []
    for nprobe in (1, 2, 4):
        for k in (1, 100, 2048):
            _check_search(oracle, h, 0, 0, Q, X, C_, lists, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
            from_lds.append(h.last_search_stats()[3])
    # nprobe = 1: three queries scan list 0 (beyond LDS), two scan list 2 (within); nprobe >= 2: all scan both lists
    assert from_lds == [2, 2, 2, 0, 0, 0, 0, 0, 0]
    h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_k_edges(oracle):
    counts = (2047, 2048, 2049)
    X, Q, C_, owner = io.edge_case(counts)
    h = _handle(X, C_)
    scanned = _check_search(oracle, h, 0, 0, Q, X, C_, owner, LB_MAX_K, 1, ctx="k 2048 nprobe 1")
    assert scanned.tolist() == list(counts)
    lab, _ = h.search(Q, LB_MAX_K, 1)
    assert lab[0, -1] == -1 and (lab[0, :-1] >= 0).all() and (lab[1:] >= 0).all()
    h.Close()
    X2, Q2, C2, owner2 = io.edge_case((5, 0, 9))  # k > n
    h = _handle(X2, C2)
    _check_search(oracle, h, 0, 0, Q2, X2, C2, owner2, 64, 3, ctx="k > n")
    h.Close()
    e = _handle(np.empty((0, 8), F), C2)  # nothing stored: all padding
    lab, dist = e.search(Q2, 7, 2)
    assert (lab == -1).all() and (dist == io.FLT_MAX).all() and e.last_search_stats() == (3, 0, 0, 0)
    e.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_adds_in_pieces_with_ids(oracle, parity):
    import torch
    from longbow_amd import ivf
    X, Q, C_, lists = parity
    rng = np.random.default_rng(7)
    ids = rng.permutation(1 << 20)[:X.shape[0]].astype(np.int64) + (np.arange(X.shape[0], dtype=np.int64) % 3 << 41)
    assert np.unique(ids).size == ids.size and (ids > 1 << 40).any()
    one = _handle(X, C_, ids=ids)
    pieces = _handle(X[:0], C_)
    dev = _handle(X[:0], C_)
    dX, dI = torch.from_numpy(X).cuda(), torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    r0 = 0
    for cnt in (1, 127, 1000, 1872):
        pieces.add(X[r0:r0 + cnt], ids[r0:r0 + cnt])
        dev.add_device(cnt, dX[r0:].data_ptr(), dI[r0:].data_ptr())
        r0 += cnt
        assert pieces.ntotal == r0 and dev.ntotal == r0
        assert np.array_equal(pieces.assignments(), lists[:r0])
        assert np.array_equal(pieces.list_sizes(), np.bincount(lists[:r0], minlength=C_.shape[0]))
    assert r0 == X.shape[0]
    want = one.search(Q, 10, 3)
    ol, od, _ = io.search(oracle, 0, 0, Q, X, C_, lists, 10, 3, ids=ids)
    assert_same(*want, ol, od, "one add, ids")
    assert_same(*pieces.search(Q, 10, 3), *want, "adds in pieces")
    assert_same(*dev.search(Q, 10, 3), *want, "device-pointer adds")
    assert np.array_equal(dev.assignments(), lists) and np.array_equal(dev.list_sizes(), one.list_sizes())
    # the device-pointer search
    dQ = torch.from_numpy(Q).cuda()
    dD = torch.full((Q.shape[0], 10), -5.0, dtype=torch.float32, device="cuda")
    dL = torch.full((Q.shape[0], 10), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    pieces.search_device(Q.shape[0], dQ.data_ptr(), 10, 3, dD.data_ptr(), dL.data_ptr())
    assert_same(dL.cpu().numpy(), dD.cpu().numpy(), *want, "device-pointer search")
    # ids on every add or on none
    for h, bad in ((pieces, None), (_handle(X[:5], C_), ids[:3])):
        before = h.ntotal
        rc = h._lib.lb_gpu_ivf_add(h._h, 3, X.ctypes.data, bad.ctypes.data if bad is not None else None)
        assert rc == INVALID and h.ntotal == before
        with pytest.raises(ivf._lib.LongbowGPUError, match="ids"):
            h.add(X[:3], bad)
        assert h.ntotal == before
    assert_same(*pieces.search(Q, 10, 3), *want, "after the refused add")
    for h in (one, pieces, dev):
        h.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_batches_and_concurrent_searches(oracle, parity):
    X, Q, C_, lists = parity
    rng = np.random.default_rng(8)
    big = rng.standard_normal((1025, X.shape[1])).astype(F)
    h = _handle(X, C_)
    ol, od, scanned = io.search(oracle, 0, 0, big, X, C_, lists, 10, 3)
    for nq in (1, 2, 1025):
        lab, dist = h.search(big[:nq], 10, 3)
        assert_same(lab, dist, ol[:nq], od[:nq], f"nq {nq}")
        assert h.last_search_stats()[:2] == (nq, int(scanned[:nq].sum()))
    out = [None] * 4

    def work(t):
        out[t] = h.search(big[t * 50:t * 50 + 200], 10, 3)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for t in range(4):
        assert_same(*out[t], ol[t * 50:t * 50 + 200], od[t * 50:t * 50 + 200], f"thread {t}")
    h.Close()


def test_profiled_search_over_two_batches(oracle):
    """1025 queries run as two batches.  A profiled search records an event between the steps of each and drains after each: it
    returns what the unprofiled search returns, and the four slots (probes, plan, scan, select) sum over the batches."""
    X, Q, C_ = io.parity_case(3000, 16, 8, 1025, seed=1238)  # (the rows of tests/test_gpu_ivfpq.py's eight_lists)
    lists = io.assign(oracle, 0, 0, X, C_)
    h = _handle(X, C_)
    want = h.search(Q, 10, 3)
    stats = h.last_search_stats()
    assert h.last_timing() == (0.0, 0.0, 0.0, 0.0) and h.last_build_timing() == 0.0
    h.set_profiling(True)
    scanned = _check_search(oracle, h, 0, 0, Q, X, C_, lists, 10, 3, ctx="profiled")
    assert scanned.size == 1025
    assert_same(*h.search(Q, 10, 3), *want, "profiled against unprofiled")
    assert h.last_search_stats() == stats
    ms = h.last_timing()
    assert len(ms) == 4 and all(np.isfinite(t) and t >= 0 for t in ms) and sum(ms) > 0, ms
    h.set_filter((np.arange(X.shape[0]) % 2 == 0).astype(np.uint8))  # the visible lists are built under profiling too
    assert h.nvisible() == X.shape[0] // 2
    ms = h.last_build_timing()
    assert np.isfinite(ms) and ms > 0, ms
    h.Close()


def test_more_probes_than_the_coarse_search_returns(oracle):
    """2100 lists are more than the LB_MAX_K probes the coarse search returns: fewer than all of them is refused before the device
    is touched, and with all of them probed the probes are the lists"""
    X, Q, C_ = io.parity_case(5000, 8, 2100, 5, seed=90)
    lists = io.assign(oracle, 0, 0, X, C_)
    h = _handle(X, C_)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.list_sizes(), np.bincount(lists, minlength=2100))
    dist = np.full((5, 10), 9.0, F)
    lab = np.full((5, 10), 77, np.int64)
    assert h._lib.lb_gpu_ivf_search(h._h, 5, Q.ctypes.data, 10, 2099, dist.ctypes.data, lab.ctypes.data) == UNSUPPORTED
    assert b"nprobe" in h._lib.lb_gpu_ivf_last_error(h._h)
    assert (dist == 9.0).all() and (lab == 77).all()
    flat = new_index(8, 0, 0)
    flat.Add(None, X)
    fl, fd = flat.SearchBatch(Q, 10)
    flat.Close()
    for nprobe in (2100, 5000):
        lab, dist = h.search(Q, 10, nprobe)
        assert_same(lab, dist, fl, fd, f"nprobe {nprobe}")
        assert h.last_search_stats() == (5, 5 * 5000, 5000, 5)
    _check_search(oracle, h, 0, 0, Q, X, C_, lists, 10, 40, ctx="nprobe 40 of 2100")
    h.Close()


def test_more_pairs_than_one_grid_dimension(oracle):
    """1024 queries x 33 probes = 33,792 (query, probe) pairs: more than the 32,768 the list scan lays along grid dimension y,
    so the rest go along z.  64 lists of ten rows: the grid is the point, not the rows."""
    X, Q, C_ = io.parity_case(n=640, dim=8, nlist=64, nq=1024, seed=88)
    lists = io.assign(oracle, 0, 0, X, C_)
    h = _handle(X, C_)
    assert np.array_equal(h.assignments(), lists)
    _check_search(oracle, h, 0, 0, Q, X, C_, lists, 5, 33, ctx="33,792 pairs")
    h.Close()


def test_batch_bounded_by_the_key_scratch():
    """One list of 4.2M rows: a query's keys are 33.6 MB, so the 1 GiB of key scratch holds 31 queries and 40 queries run as two
    batches although they are fewer than 1024.  Every list is probed: the flat index on the same rows is the comparator."""
    gpu_or_skip()
    rng = np.random.default_rng(89)
    n, dim, nq = 4_200_000, 4, 40
    X = rng.standard_normal((n, dim)).astype(F)
    Q = rng.standard_normal((nq, dim)).astype(F)
    h = _handle(X, np.zeros((1, dim), F))
    assert h.list_sizes().tolist() == [n]
    flat = new_index(dim, 0, 0)
    flat.Add(None, X)
    lab, dist = h.search(Q, 10, 1)
    assert_same(lab, dist, *flat.SearchBatch(Q, 10), "two scratch-bounded batches")
    assert h.last_search_stats() == (nq, nq * n, n, 0)
    flat.Close()
    h.Close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_non_finite_values(metric):
    """The comparator is an independent, existing implementation of "exact k-NN among these rows": the flat f32 index under a
    row filter that leaves the rows of the probed lists (the numpy oracle's NaN order is not pinned)."""
    rng = np.random.default_rng(9)
    n, dim, nlist, nprobe, k = 700, 12, 6, 3, 700  # k = n: every row of the probed lists is reported, the special ones too
    X = rng.standard_normal((n, dim)).astype(F)
    C_ = X[[3, 100, 200, 300, 400, 500]].copy()
    X[17, 4] = np.nan
    X[18, 0] = np.inf
    X[19] = 0.0
    Q = rng.standard_normal((4, dim)).astype(F)
    Q[3, 2] = np.nan
    for order in (0, 1):
        h = _handle(X, C_, metric, order)
        lists = h.assignments()
        assert np.array_equal(h.list_sizes(), np.bincount(lists, minlength=nlist))
        cent = new_index(dim, metric, order)
        cent.Add(None, C_)
        pr, _ = cent.SearchBatch(Q, nprobe)
        lab, dist = h.search(Q, k, nprobe)
        flat = new_index(dim, metric, order)
        flat.Add(None, X)
        for j in range(Q.shape[0]):
            flat.set_filter(np.isin(lists, pr[j]).astype(np.uint8))
            fl, fd = flat.SearchBatch(Q[j:j + 1], k)
            assert np.array_equal(lab[j], fl[0]), (metric, order, j, lab[j], fl[0])
            assert np.array_equal(dist[j], fd[0], equal_nan=True), (metric, order, j)
        assert {17, 18, 19} <= set(lab.reshape(-1).tolist())  # (the special rows do reach the lists)
        for x in (cent, flat, h):
            x.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_refusals_behind_a_live_handle(parity):
    from longbow_amd import gpu
    X, Q, C_, _ = parity
    h = _handle(X, C_)
    lib = h._lib
    kmax = LB_MAX_K + 1
    dist = np.full((Q.shape[0], kmax), 9.0, F)
    lab = np.full((Q.shape[0], kmax), 77, np.int64)
    args = (Q.shape[0], Q.ctypes.data)
    assert lib.lb_gpu_ivf_search(h._h, *args, kmax, 3, dist.ctypes.data, lab.ctypes.data) == UNSUPPORTED
    assert b"2048" in lib.lb_gpu_ivf_last_error(h._h)
    assert lib.lb_gpu_ivf_search(h._h, *args, 10, 0, dist.ctypes.data, lab.ctypes.data) == INVALID
    assert b"nprobe" in lib.lb_gpu_ivf_last_error(h._h)
    assert lib.lb_gpu_ivf_search(h._h, *args, 10, -4, dist.ctypes.data, lab.ctypes.data) == INVALID
    assert lib.lb_gpu_ivf_search(h._h, *args, 0, 3, dist.ctypes.data, lab.ctypes.data) == INVALID
    c = gpu.Cancel()
    c.fire()
    assert lib.lb_gpu_ivf_search_ctx(h._h, *args, 10, 3, dist.ctypes.data, lab.ctypes.data, c._h) == CANCELLED
    assert lib.lb_gpu_ivf_assignments(h._h, X.shape[0] - 1, 2, lab.ctypes.data) == INVALID
    assert (dist == 9.0).all() and (lab == 77).all()
    st = (C.c_int64 * 4)()
    assert lib.lb_gpu_ivf_last_search_stats(h._h, st) == 0
    assert h.hbm_bytes >= X.nbytes + C_.nbytes
    h.reserve(10000)
    assert h.ntotal == X.shape[0] and h.search(Q[:2], 5, 3)[0].shape == (2, 5)
    h.Close()


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_python_mirror(oracle, parity):
    from longbow_amd import ivf
    X, Q, C_, lists = parity
    h = _handle(X, C_)
    want = h.search(Q, 10, 3)
    idx = ivf.IVFFlatIndex(X.shape[1], ivf.IVFFlatConfig(NClusters=16, NProbe=3), centroids=C_)
    assert idx.Type() == "ivf_flat" and idx.Dimension() == X.shape[1] and idx.NeedsBuild() is True and idx.Size() == 0
    idx.AddBatch(np.arange(2000), X[:2000])
    idx.Add(2000, X[2000])
    assert idx.Size() == idx.Len() == 2001
    with pytest.raises(RuntimeError):
        idx.Search(Q[0], 10)
    idx.Build()
    idx.AddBatch(np.arange(2001, X.shape[0]), X[2001:])  # after Build(): straight to the handle
    assert idx.Size() == X.shape[0]
    assert_same(*idx.SearchBatch(Q, 10), *want, "SearchBatch")
    ids, dist = idx.Search(Q[5], 10)
    assert np.array_equal(ids, want[0][5]) and np.array_equal(dist, want[1][5])
    assert_same(*idx.SearchBatch(Q, 10, nprobe=16), *h.search(Q, 10, 16), "nprobe=")
    assert np.array_equal(idx.list_sizes(), h.list_sizes()) and np.array_equal(idx.assignments(), lists)
    assert idx.last_search_stats()[0] == Q.shape[0]
    for call in (idx.Save, idx.Load):
        with pytest.raises(NotImplementedError):
            call("ivf.bin")
    idx.Close()
    h.Close()
    # Build() without centroids trains them on the buffered rows
    t = ivf.IVFFlatIndex(X.shape[1], ivf.IVFFlatConfig(NClusters=8, NProbe=8), train_iters=2)
    t.AddBatch(np.arange(500), X[:500])
    t.Build()
    flat = new_index(X.shape[1], 0, 0)
    flat.Add(None, X[:500])
    assert_same(*t.SearchBatch(Q, 5), *flat.SearchBatch(Q, 5), "trained, every list probed")
    flat.Close()
    t.Close()


def test_train_is_train_kmeans():
    """the templated 16 form; tests/test_gpu_coarse_train.py holds ivf.train at the shapes a coarse quantiser has"""
    from longbow_amd import ivf
    gpu_or_skip()
    rng = np.random.default_rng(11)
    X = rng.standard_normal((2000, 16)).astype(F)
    rows = rng.permutation(2000)[:8].astype(np.int64)
    want, _ = ko.train_kmeans(X, 8, 5, rows)
    got = ivf.train(X, 8, max_iter=5, init_rows=rows)
    assert got.shape == (8, 16) and got.tobytes() == np.ascontiguousarray(want, F).tobytes()
    assert ivf.train(X, 8, max_iter=0, init_rows=rows).tobytes() == X[rows].tobytes()
