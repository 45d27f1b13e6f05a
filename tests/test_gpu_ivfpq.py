"""lb_gpu_ivfpq_* on the GPU against tests/ivfpq_oracle.py (the semantics restated over the C oracle's batch_flat, pq_encode,
build_adc_table, adc_batch and topk_canonical): labels and distances must be equal, bit for bit.  The shapes are the smallest at
which the kernels can still go wrong: the byte and the 16-byte forms of the scan and of the list-major copy, lists around the
1024-position tile, a list that needs the tile stride loop, list boundaries inside a wave, selections within LDS and beyond it,
the workload's table, the largest table (with the segments beside it in LDS and not), more queries than a batch."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import ivfpq_oracle as pqo
from tests import ivf_piece_cases as pc
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED, CANCELLED = 1, 6, 8
LB_MAX_K = 2048
LDS_KEYS = 16384  # IVF_SELECT_LDS_KEYS: a query with more scanned rows is selected from global memory


def _handle(X, C_, cb, order=0, ids=None):
    from longbow_amd import ivfpq
    gpu_or_skip()
    h = ivfpq.IVFPQ(pqo.blob(cb), C_, order)
    if X.shape[0]:
        h.add(X, ids)
    return h


def _check_search(oracle, h, cb, order, Q, C_, lists, codes, k, nprobe, ids=None, ctx=""):
    ol, od, scanned = pqo.search(oracle, cb, order, Q, C_, lists, codes, k, nprobe, ids=ids)
    lab, dist = h.search(Q, k, nprobe)
    assert_same(lab, dist, ol, od, ctx)
    st = h.last_search_stats()
    assert st[0] == Q.shape[0] and st[1] == int(scanned.sum()) and st[2] == int(scanned.max()), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= LDS_KEYS).sum()), (st, ctx)
    return scanned


def _pq_handle(cb, codes):
    from longbow_amd import pq
    enc = pq.PQEncoder(pqo.blob(cb))
    enc.add_codes(codes)
    return enc


@pytest.fixture(scope="module")
def parity(oracle):
    """the byte-form shape of case 1 with its oracle lists and codes at order 0 (shared by the ties, adds, batches and refusals)"""
    X, Q, C_, cb = pqo.parity_case(*pqo.PARITY_SHAPES[0])
    return X, Q, C_, cb, pqo.assign(oracle, 0, X, C_), pqo.encode(oracle, cb, X)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dims,M", pqo.PARITY_SHAPES)
def test_parity_grid(oracle, dims, M, order):
    X, Q, C_, cb = pqo.parity_case(dims, M)
    lists, codes = pqo.assign(oracle, order, X, C_), pqo.encode(oracle, cb, X)
    h = _handle(X, C_, cb, order)
    assert h.ntotal == X.shape[0] and (h.nlist, h.dims) == C_.shape and h.m == M and h.order == order
    assert np.array_equal(h.assignments(), lists)
    assert np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    assert np.array_equal(h.codes(), codes) and np.array_equal(h.codes(100, 7), codes[100:107])
    assert np.array_equal(h.centroids(), C_)
    for nprobe in (1, 3, 16):
        _check_search(oracle, h, cb, order, Q, C_, lists, codes, 10, nprobe, ctx=f"dims {dims} M {M} order {order} nprobe {nprobe}")
    h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,M,n", [(16, 4, 3000), (32, 16, 3000), (32, 16, 70000)])
def test_every_list_probed_equals_the_pq_handle(dims, M, n):
    """70,000 rows: the PQ handle's sampled threshold and, with it, its byte-table prefilter are in play"""
    X, Q, C_, cb = pqo.parity_case(dims, M, n=n)
    rng = np.random.default_rng(2)
    ids = rng.permutation(1 << 22)[:n].astype(np.int64) + (1 << 41)
    for with_ids in (False, True):
        h = _handle(X, C_, cb, ids=ids if with_ids else None)
        enc = _pq_handle(cb, h.codes())
        for prefilter in (True, False):
            enc.set_prefilter(prefilter)
            fl, fd = enc.Search(Q, 10)
            if with_ids:
                fl = ids[fl]
            for nprobe in (16, 21):
                lab, dist = h.search(Q, 10, nprobe)
                assert_same(lab, dist, fl, fd, f"dims {dims} M {M} n {n} ids {with_ids} prefilter {prefilter} nprobe {nprobe}")
                assert h.last_search_stats()[1] == Q.shape[0] * n
        enc.Close()
        h.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_ties_come_in_row_order(oracle, parity):
    X, Q, C_, cb, lists, codes = parity
    X3, lists3, codes3 = np.concatenate((X, X, X)), np.tile(lists, 3), np.tile(codes, (3, 1))
    n = X.shape[0]
    h = _handle(X3, C_, cb)
    assert np.array_equal(h.codes(), codes3) and np.array_equal(h.assignments(), lists3)
    for nprobe in (2, 16):
        _check_search(oracle, h, cb, 0, Q, C_, lists3, codes3, 10, nprobe, ctx=f"ties nprobe {nprobe}")
    lab, dist = h.search(Q, 10, 16)
    assert (dist[:, 0] == dist[:, 1]).all() and (dist[:, 1] == dist[:, 2]).all()
    assert (lab[:, 0] < n).all() and (lab[:, 1] == lab[:, 0] + n).all() and (lab[:, 2] == lab[:, 0] + 2 * n).all()
    assert (lab[:, 9] < n).all()  # k = 10 cuts the fourth group after its lowest row
    h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_list_length_edges(oracle):
    """tests/test_ivfpq_semantics.py asserts of this input what the case needs: the counts, the stride loop's second step at
    nprobe = 1 and several list boundaries inside one wave with every list probed"""
    X, Q, C_, owner, cb = pqo.edge_case()
    codes = pqo.encode(oracle, cb, X)
    h = _handle(X, C_, cb)
    assert np.array_equal(h.assignments(), owner) and h.list_sizes().tolist() == list(pqo.EDGE_COUNTS)
    assert np.array_equal(h.codes(), codes)
    nlist = C_.shape[0]
    for nprobe, k in ((1, 10), (1, 200), (2, 10), (5, 200), (nlist, 10), (nlist, 200)):
        _check_search(oracle, h, cb, 0, Q, C_, owner, codes, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
    lab, dist = h.search(Q, 10, 1)
    assert (lab[0] == -1).all() and (dist[0] == pqo.FLT_MAX).all()  # an empty probed list: all padding
    assert lab[1, 0] == np.flatnonzero(owner == 1)[0] and (lab[1, 1:] == -1).all() and (dist[1, 1:] == pqo.FLT_MAX).all()  # P_q < k
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_the_long_selection(oracle):
    X, Q, C_, cb = pqo.skew_case()
    lists, codes = pqo.assign(oracle, 0, X, C_), pqo.encode(oracle, cb, X)
    h = _handle(X, C_, cb)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.codes(), codes)
    from_lds = []
    for nprobe in (1, 4):
        for k in (1, 100, 2048):
            scanned = _check_search(oracle, h, cb, 0, Q, C_, lists, codes, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
            from_lds.append(h.last_search_stats()[3])
    assert scanned.min() > LDS_KEYS
    # nprobe = 1: three queries scan list 0 (beyond LDS), two scan list 2 (within); nprobe = 4: all scan both lists
    assert from_lds == [2, 2, 2, 0, 0, 0]
    h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,M,n,nlist,nprobes", [
    (192, 96, 2000, 8, (2, 8)),      # the workload's table: 98,304 B of LDS
    (159, 159, 500, 130, (2, 129)),  # the largest table: 162,816 B; 129 probes' segments no longer fit beside it
    (4, 1, 1000, 8, (2, 8)),
    (80, 80, 700, 8, (3,)),          # M % 16 == 0 without a compile-time form
])
def test_table_sizes(oracle, dims, M, n, nlist, nprobes):
    X, Q, C_, cb = pqo.parity_case(dims, M, n=n, nlist=nlist, nq=5)
    lists, codes = pqo.assign(oracle, 0, X, C_), pqo.encode(oracle, cb, X)
    h = _handle(X, C_, cb)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.codes(), codes)
    for nprobe in nprobes:
        _check_search(oracle, h, cb, 0, Q, C_, lists, codes, 10, nprobe, ctx=f"M {M} nprobe {nprobe}")
    h.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_adds_in_pieces_with_ids(oracle, parity):
    import torch
    from longbow_amd import ivfpq
    X, Q, C_, cb, lists, codes = parity
    rng = np.random.default_rng(7)
    ids = rng.permutation(1 << 20)[:X.shape[0]].astype(np.int64) + (np.arange(X.shape[0], dtype=np.int64) % 3 << 41)
    one = _handle(X, C_, cb, ids=ids)
    pieces = _handle(X[:0], C_, cb)
    dev = _handle(X[:0], C_, cb)
    dX, dI = torch.from_numpy(X).cuda(), torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    r0 = 0
    for cnt in (127, 1000, 1873):
        pieces.add(X[r0:r0 + cnt], ids[r0:r0 + cnt])
        dev.add_device(cnt, dX[r0:].data_ptr(), dI[r0:].data_ptr())
        r0 += cnt
        assert pieces.ntotal == r0 and dev.ntotal == r0
        assert np.array_equal(pieces.assignments(), lists[:r0]) and np.array_equal(pieces.codes(), codes[:r0])
        assert np.array_equal(pieces.list_sizes(), np.bincount(lists[:r0], minlength=C_.shape[0]))
        # a search between the adds sees exactly the committed rows
        _check_search(oracle, pieces, cb, 0, Q[:5], C_, lists[:r0], codes[:r0], 10, 3, ids=ids, ctx=f"after {r0} rows")
    assert r0 == X.shape[0]
    want = one.search(Q, 10, 3)
    ol, od, _ = pqo.search(oracle, cb, 0, Q, C_, lists, codes, 10, 3, ids=ids)
    assert_same(*want, ol, od, "one add, ids")
    assert_same(*pieces.search(Q, 10, 3), *want, "adds in pieces")
    assert_same(*dev.search(Q, 10, 3), *want, "device-pointer adds")
    assert np.array_equal(dev.assignments(), lists) and np.array_equal(dev.codes(), codes)
    # the device-pointer search
    dQ = torch.from_numpy(Q).cuda()
    dD = torch.full((Q.shape[0], 10), -5.0, dtype=torch.float32, device="cuda")
    dL = torch.full((Q.shape[0], 10), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    pieces.search_device(Q.shape[0], dQ.data_ptr(), 10, 3, dD.data_ptr(), dL.data_ptr())
    assert_same(dL.cpu().numpy(), dD.cpu().numpy(), *want, "device-pointer search")
    # ids on every add or on none
    for h, bad in ((pieces, None), (_handle(X[:5], C_, cb), ids[:3])):
        before = h.ntotal
        rc = h._lib.lb_gpu_ivfpq_add(h._h, 3, X.ctypes.data, bad.ctypes.data if bad is not None else None)
        assert rc == INVALID and h.ntotal == before
        with pytest.raises(ivfpq._lib.LongbowGPUError, match="ids"):
            h.add(X[:3], bad)
        assert h.ntotal == before
    assert_same(*pieces.search(Q, 10, 3), *want, "after the refused add")
    # reserve changes nothing
    hbm = pieces.hbm_bytes
    pieces.reserve(20000)
    assert pieces.ntotal == X.shape[0] and pieces.hbm_bytes > hbm
    assert np.array_equal(pieces.codes(), codes) and np.array_equal(pieces.assignments(), lists)
    assert_same(*pieces.search(Q, 10, 3), *want, "after reserve")
    pieces.add(X[:10], ids[:10])  # and the handle goes on taking rows
    assert pieces.ntotal == X.shape[0] + 10 and np.array_equal(pieces.codes(X.shape[0]), codes[:10])
    for h in (one, pieces, dev):
        h.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_batches_and_concurrent_searches(oracle, parity):
    X, Q, C_, cb, lists, codes = parity
    rng = np.random.default_rng(8)
    big = rng.standard_normal((1025, X.shape[1])).astype(F)
    h = _handle(X, C_, cb)
    ol, od, scanned = pqo.search(oracle, cb, 0, big, C_, lists, codes, 10, 3)
    for nq in (1, 1025):
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


@pytest.fixture(scope="module")
def eight_lists(oracle):
    """3000 rows of 16 dimensions over 8 lists, M = 4, with the oracle's lists at order 0 and codes: the rows of
    tests/test_gpu_ivf.py's profiled search"""
    X, _, C_, cb = pqo.parity_case(16, 4, n=3000, nlist=8)
    return X, C_, cb, pqo.assign(oracle, 0, X, C_), pqo.encode(oracle, cb, X)


def test_profiled_search_over_two_batches(oracle, eight_lists):
    """1025 queries run as two batches.  A profiled search records an event between the steps of each and drains after each: it
    returns what the unprofiled search returns, and the five slots (probes, plan, tables, scan, select) sum over the batches."""
    X, C_, cb, lists, codes = eight_lists
    Q = np.random.default_rng(8).standard_normal((1025, X.shape[1])).astype(F)
    h = _handle(X, C_, cb)
    want = h.search(Q, 10, 3)
    stats = h.last_search_stats()
    assert h.last_timing() == (0.0,) * 5
    h.set_profiling(True)
    scanned = _check_search(oracle, h, cb, 0, Q, C_, lists, codes, 10, 3, ctx="profiled")
    assert scanned.size == 1025
    assert_same(*h.search(Q, 10, 3), *want, "profiled against unprofiled")
    assert h.last_search_stats() == stats
    ms = h.last_timing()
    assert len(ms) == 5 and all(np.isfinite(t) and t >= 0 for t in ms) and sum(ms) > 0, ms
    h.Close()


@pytest.mark.parametrize("order", [0, 1])
def test_the_partition_is_the_ivf_flat_handle_s(oracle, eight_lists, order):
    """the same centroids and rows, added in three pieces with ids: both handles hold the partition the oracle assigns"""
    from longbow_amd import ivf
    X, C_, cb, lists, _ = eight_lists
    if order:
        lists = pqo.assign(oracle, order, X, C_)
    ids = np.random.default_rng(12).permutation(1 << 20)[:X.shape[0]].astype(np.int64) + (1 << 41)
    codes_h = _handle(X[:0], C_, cb, order)
    rows_h = ivf.IVFFlat(C_, 0, order)
    r0 = 0
    for cnt in (127, 1000, 1873):
        for h in (codes_h, rows_h):
            h.add(X[r0:r0 + cnt], ids[r0:r0 + cnt])
        r0 += cnt
    assert r0 == X.shape[0] and codes_h.ntotal == rows_h.ntotal == r0
    assert np.array_equal(codes_h.assignments(), lists) and np.array_equal(rows_h.assignments(), lists)
    sizes = np.bincount(lists, minlength=C_.shape[0])
    assert np.array_equal(codes_h.list_sizes(), sizes) and np.array_equal(rows_h.list_sizes(), sizes)
    for h in (codes_h, rows_h):
        h.Close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_every_list_probed_without_the_coarse_search(oracle):
    """2100 lists are more than the LB_MAX_K probes the coarse search returns: with all of them probed the probes are the lists"""
    X, Q, C_, cb = pqo.parity_case(8, 4, n=5000, nlist=2100, nq=5)
    lists, codes = pqo.assign(oracle, 0, X, C_), pqo.encode(oracle, cb, X)
    h = _handle(X, C_, cb)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.list_sizes(), np.bincount(lists, minlength=2100))
    bl, bd = pqo.brute(oracle, cb, Q, codes, 10)
    for nprobe in (2100, 5000):
        lab, dist = h.search(Q, 10, nprobe)
        assert_same(lab, dist, bl, bd, f"nprobe {nprobe}")
        assert h.last_search_stats() == (5, 5 * 5000, 5000, 5)
    _check_search(oracle, h, cb, 0, Q, C_, lists, codes, 10, 40, ctx="nprobe 40 of 2100")
    dist = np.full((5, 10), 9.0, F)
    lab = np.full((5, 10), 77, np.int64)
    assert h._lib.lb_gpu_ivfpq_search(h._h, 5, Q.ctypes.data, 10, 2099, dist.ctypes.data, lab.ctypes.data) == UNSUPPORTED
    assert (dist == 9.0).all() and (lab == 77).all()
    h.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_refusals_behind_a_live_handle(parity):
    from longbow_amd import gpu
    X, Q, C_, cb, lists, codes = parity
    h = _handle(X, C_, cb)
    lib = h._lib
    kmax = LB_MAX_K + 1
    dist = np.full((Q.shape[0], kmax), 9.0, F)
    lab = np.full((Q.shape[0], kmax), 77, np.int64)
    u8 = np.full(8, 0xA5, np.uint8)
    args = (Q.shape[0], Q.ctypes.data)
    assert lib.lb_gpu_ivfpq_search(h._h, *args, kmax, 3, dist.ctypes.data, lab.ctypes.data) == UNSUPPORTED
    assert b"2048" in lib.lb_gpu_ivfpq_last_error(h._h)
    assert lib.lb_gpu_ivfpq_search(h._h, *args, 10, 0, dist.ctypes.data, lab.ctypes.data) == INVALID
    assert b"nprobe" in lib.lb_gpu_ivfpq_last_error(h._h)
    assert lib.lb_gpu_ivfpq_search(h._h, *args, 10, -4, dist.ctypes.data, lab.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfpq_search(h._h, *args, 0, 3, dist.ctypes.data, lab.ctypes.data) == INVALID
    c = gpu.Cancel()
    c.fire()
    assert lib.lb_gpu_ivfpq_search_ctx(h._h, *args, 10, 3, dist.ctypes.data, lab.ctypes.data, c._h) == CANCELLED
    assert lib.lb_gpu_ivfpq_assignments(h._h, X.shape[0] - 1, 2, lab.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfpq_get_codes(h._h, X.shape[0] - 1, 2, u8.ctypes.data) == INVALID
    assert (dist == 9.0).all() and (lab == 77).all() and (u8 == 0xA5).all()
    st = (C.c_int64 * 4)()
    assert lib.lb_gpu_ivfpq_last_search_stats(h._h, st) == 0
    # codes three times, lists, assignments: what a row costs, plus the codebooks and the centroids
    n, M = X.shape[0], cb.shape[0]
    assert h.hbm_bytes >= n * (3 * M + 12) + cb.nbytes + C_.nbytes
    h.set_profiling(True)
    h.search(Q, 10, 3)
    ms = h.last_timing()
    assert len(ms) == 5 and all(t >= 0 for t in ms) and sum(ms) > 0
    h.Close()
    e = _handle(X[:0], C_, cb)  # nothing stored: all padding
    el, ed = e.search(Q, 7, 2)
    assert (el == -1).all() and (ed == pqo.FLT_MAX).all() and e.last_search_stats() == (Q.shape[0], 0, 0, 0)
    assert e.codes().shape == (0, cb.shape[0]) and e.list_sizes().sum() == 0
    e.Close()


def test_python_front_end(parity):
    from longbow_amd import ivfpq, pq
    X, Q, C_, cb, lists, codes = parity
    enc = pq.PQEncoder(pqo.blob(cb))
    h = ivfpq.IVFPQ(enc, C_)  # the codebooks of an encoder
    h.add(X)
    assert np.array_equal(h.codes(), codes) and np.array_equal(h.codes(), enc.Encode(X))
    h.Close()
    enc.Close()
    cent, blob = ivfpq.train(X[:1500], 8, 4, max_iter=2, seed=3)
    assert cent.shape == (8, X.shape[1]) and len(blob) == 12 + 4 * 256 * (X.shape[1] // 4) * 4
    t = ivfpq.IVFPQ(blob, cent)
    t.add(X[:1500])
    enc = pq.PQEncoder(blob)
    enc.add_codes(t.codes())
    assert_same(*t.search(Q, 5, 8), *enc.Search(Q, 5), "trained, every list probed")
    enc.Close()
    t.Close()


# the shared add across two pieces (tests/ivf_piece_cases.py) ----------------------------------------------------------------
@pytest.fixture(scope="module")
def two_pieces(oracle):
    """the case with random codebooks (M = 128: the most subspaces that divide 8192 within the table limit), a maker of empty
    handles over it, the snapshot of one filled by small adds and the oracle's assignment"""
    gpu_or_skip()
    X, ids, C_, Q = pc.case()
    cb = np.random.default_rng(21).standard_normal((128, 256, pc.DIMS // 128)).astype(F) * F(0.3)
    new = lambda: _handle(X[:0], C_, cb)
    return X, ids, Q, new, pc.reference(new, X, ids, Q), pqo.assign(oracle, 0, X, C_)


@pytest.mark.parametrize("device", [False, True])
def test_one_add_across_pieces(two_pieces, device):
    X, ids, Q, new, want, lists = two_pieces
    pc.check_one_add(new, X, ids, Q, want, lists, device)
