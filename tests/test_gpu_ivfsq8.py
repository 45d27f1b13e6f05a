"""lb_gpu_ivfsq8_* on the GPU against tests/ivfsq8_oracle.py (the semantics restated over tests/ivf_oracle.py's lists and probes
and tests/sq8_oracle.py's encode, dist_s and topk): labels and distances must be equal, bit for bit.  The shapes are the smallest
at which the kernels can still go wrong: one piece, a padded stride, a partial chunk, a full chunk plus a partial one and the
workload's row; lists around the 128-row tile, a list whose workgroups take a second tile, list boundaries inside a wave;
selections within LDS and beyond it; two S that round to one float; the largest S; more queries than a batch."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import ivfsq8_oracle as sqo
from tests import ivf_piece_cases as pc
from tests import refine_oracle as fo
from tests import row_view_cases as rv
from tests import sq8_oracle as so
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED, CANCELLED = 1, 6, 8
LB_MAX_K = 2048
LDS_KEYS = sqo.LDS_KEYS


def _handle(X, C_, mn, mx, order=0, ids=None):
    from longbow_amd import ivfsq8
    gpu_or_skip()
    h = ivfsq8.IVFSQ8(mn, mx, C_, order)
    if X.shape[0]:
        h.add(X, ids)
    return h


def _check_search(oracle, h, order, Q, C_, lists, codes, mn, mx, k, nprobe, ids=None, mask=None, ctx=""):
    ol, od, scanned = sqo.search(oracle, order, Q, C_, lists, codes, mn, mx, k, nprobe, ids=ids, mask=mask)
    lab, dist = h.search(Q, k, nprobe)
    assert_same(lab, dist, ol, od, ctx)
    st = h.last_search_stats()
    assert st[0] == Q.shape[0] and st[1] == int(scanned.sum()) and st[2] == int(scanned.max()), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= LDS_KEYS).sum()), (st, ctx)
    return scanned


def _sq8_handle(mn, mx, codes):
    from longbow_amd import sq8
    enc = sq8.SQ8Encoder(codes.shape[1])
    enc.set_bounds(mn, mx)
    enc.add_codes(codes)
    return enc


@pytest.fixture(scope="module")
def parity(oracle):
    """the one-piece shape of case 1 with its oracle lists and codes at order 0 (shared by the ties, adds, batches, refusals,
    filters and the refine)"""
    X, Q, C_, mn, mx = sqo.parity_case(16)
    return X, Q, C_, mn, mx, sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dims", sqo.PARITY_DIMS)
def test_parity_grid(oracle, dims, order):
    X, Q, C_, mn, mx = sqo.parity_case(dims)
    lists, codes = sqo.assign(oracle, order, X, C_), sqo.encode(X, mn, mx)
    h = _handle(X, C_, mn, mx, order)
    assert h.ntotal == X.shape[0] and (h.nlist, h.dims) == C_.shape and h.order == order
    assert h._lib.lb_gpu_ivfsq8_dims(h._h) == dims and h._lib.lb_gpu_ivfsq8_order(h._h) == order and h._lib.lb_gpu_ivfsq8_nlist(h._h) == 16
    assert np.array_equal(h.assignments(), lists)
    assert np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    assert np.array_equal(h.codes(), codes) and np.array_equal(h.codes(100, 7), codes[100:107])
    assert np.array_equal(h.centroids(), C_)
    bmn, bmx = h.bounds()
    assert np.array_equal(bmn, mn) and np.array_equal(bmx, mx)
    for nprobe in (1, 3, 16):
        _check_search(oracle, h, order, Q, C_, lists, codes, mn, mx, 10, nprobe, ctx=f"dims {dims} order {order} nprobe {nprobe}")
    h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [16, 20])
def test_every_list_probed_equals_the_sq8_handle(dims):
    X, Q, C_, mn, mx = sqo.parity_case(dims)
    n = X.shape[0]
    ids = np.random.default_rng(2).permutation(1 << 22)[:n].astype(np.int64) + (1 << 41)
    for with_ids in (False, True):
        h = _handle(X, C_, mn, mx, ids=ids if with_ids else None)
        enc = _sq8_handle(mn, mx, h.codes())
        fl, fd = enc.search(Q, 10)
        if with_ids:
            fl = ids[fl]
        for nprobe in (16, 21):
            lab, dist = h.search(Q, 10, nprobe)
            assert_same(lab, dist, fl, fd, f"dims {dims} ids {with_ids} nprobe {nprobe}")
            assert h.last_search_stats()[1] == Q.shape[0] * n
        enc.Close()
        h.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_ties_come_in_row_order(oracle, parity):
    X, Q, C_, mn, mx, lists, codes = parity
    X3, lists3, codes3 = np.concatenate((X, X, X)), np.tile(lists, 3), np.tile(codes, (3, 1))
    n = X.shape[0]
    h = _handle(X3, C_, mn, mx)
    assert np.array_equal(h.codes(), codes3) and np.array_equal(h.assignments(), lists3)
    for nprobe in (2, 16):
        _check_search(oracle, h, 0, Q, C_, lists3, codes3, mn, mx, 10, nprobe, ctx=f"ties nprobe {nprobe}")
    # every row comes three times with one S (and an integer S ties between different rows too): a tie group is in row order
    lab, dist = h.search(Q, 10, 16)
    tie = dist[:, 1:] == dist[:, :-1]
    assert (tie.sum(axis=1) >= 2).all() and (lab[:, 1:][tie] > lab[:, :-1][tie]).all()
    assert (dist[:, 0] == dist[:, 1]).all() and (dist[:, 1] == dist[:, 2]).all()
    for j in range(Q.shape[0]):  # the best row's three copies are all among the best S
        best = lab[j][dist[j] == dist[j, 0]]
        assert {int(best[0]) % n + i * n for i in range(3)} <= set(best.tolist()) or best.size == 10
    h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_the_order_is_the_integers_not_the_floats(oracle):
    """tests/test_ivfsq8_semantics.py asserts of this input that S = 2^24 + 1, 2^24, 2^24 + 1, 2^24 and that all four are one
    float: a selection keyed by (float32(S), row) would answer [0, 1, 2, 3]"""
    X, Q, C_, mn, mx = sqo.rounding_case()
    lists, codes = sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)
    h = _handle(X, C_, mn, mx)
    assert np.array_equal(h.codes(), codes) and np.array_equal(h.assignments(), lists)
    lab, dist = h.search(Q, 4, 2)
    assert lab[0].tolist() == [1, 3, 0, 2] and (dist[0] == F(16777216.0)).all()
    _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, 4, 2, ctx="rounding case")
    enc = _sq8_handle(mn, mx, codes)
    assert_same(lab, dist, *enc.search(Q, 4), "rounding case against the flat SQ8 handle")
    enc.Close()
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_list_length_edges(oracle):
    """tests/test_ivfsq8_semantics.py asserts of this input what the case needs: the counts, a workgroup's second tile at
    nprobe = 1 and several list boundaries inside one wave with every list probed"""
    X, Q, C_, owner, mn, mx = sqo.edge_case()
    codes = sqo.encode(X, mn, mx)
    h = _handle(X, C_, mn, mx)
    assert np.array_equal(h.assignments(), owner) and h.list_sizes().tolist() == list(sqo.EDGE_COUNTS)
    assert np.array_equal(h.codes(), codes)
    nlist = C_.shape[0]
    for nprobe, k in ((1, 10), (1, 200), (2, 10), (5, 200), (nlist, 10), (nlist, 200)):
        _check_search(oracle, h, 0, Q, C_, owner, codes, mn, mx, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
    lab, dist = h.search(Q, 10, 1)
    assert (lab[0] == -1).all() and (dist[0] == sqo.FLT_MAX).all()  # an empty probed list: all padding
    assert lab[1, 0] == np.flatnonzero(owner == 1)[0] and (lab[1, 1:] == -1).all() and (dist[1, 1:] == sqo.FLT_MAX).all()  # P_q < k
    h.Close()


def test_one_workgroup_walks_several_tiles_and_chunks(oracle):
    """1024 queries x 4 probes = 4,096 pairs, so the scan's grid has one workgroup per (query, list): it walks the three or more
    128-row tiles of the longest list, the last one partial, in two chunks each (136 dims at a stride of 144 bytes: nine pieces,
    8 + 1), and the pipeline wraps from a tile's last chunk to the next tile's first"""
    nq, nprobe, dims = 1024, 4, 136
    X, Q, C_, mn, mx = sqo.parity_case(dims, n=2400, nlist=8, nq=nq)
    lists, codes = sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)
    big = int(np.bincount(lists, minlength=8).max())
    pieces = -(-dims // 16)
    assert sqo.scan_tiles_x(nq * nprobe, big) == 1
    assert big > 2 * sqo.TILE and big % sqo.TILE != 0, big
    assert -(-pieces // sqo.CHUNK) >= 2 and pieces % sqo.CHUNK != 0
    h = _handle(X, C_, mn, mx)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.codes(), codes)
    _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, 10, nprobe, ctx="several tiles and chunks")
    h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_the_long_selection(oracle):
    X, Q, C_, mn, mx = sqo.skew_case()
    lists, codes = sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)
    h = _handle(X, C_, mn, mx)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.codes(), codes)
    from_lds = []
    for nprobe in (1, 4):
        for k in (1, 100, 2048):
            scanned = _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
            from_lds.append(h.last_search_stats()[3])
    assert scanned.min() > LDS_KEYS
    # nprobe = 1: three queries scan list 0 (beyond LDS), two scan list 2 (within); nprobe = 4: all scan both lists
    assert from_lds == [2, 2, 2, 0, 0, 0]
    h.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_the_largest_s(oracle):
    """dims 8192, bounds 0 / 1: a row all 0 (code 0) against a query all at max (code 255) is S = 8192 * 65025, the largest the
    arithmetic meets, among ordinary rows"""
    dims, n = 8192, 300
    rng = np.random.default_rng(81)
    X = rng.random((n, dims), dtype=F)
    X[17] = 0.0
    X[200] = 1.0
    Q = np.concatenate((np.ones((1, dims), F), np.zeros((1, dims), F), rng.random((2, dims), dtype=F)))
    C_ = X[[3, 50, 120, 250]].copy()
    mn, mx = np.zeros(dims, F), np.ones(dims, F)
    lists, codes = sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)
    assert not codes[17].any() and (codes[200] == 255).all()
    h = _handle(X, C_, mn, mx)
    assert np.array_equal(h.codes(), codes) and np.array_equal(h.assignments(), lists)
    for nprobe in (2, 4):
        _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, n, nprobe, ctx=f"dims 8192 nprobe {nprobe}")
    lab, dist = h.search(Q[:2], n, 4)
    assert lab[0, -1] == 17 and dist[0, -1] == F(8192 * 65025) and lab[1, -1] == 200 and dist[1, -1] == F(8192 * 65025)
    assert lab[0, 0] == 200 and dist[0, 0] == 0.0
    h.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_adds_in_pieces_with_ids(oracle, parity):
    import torch
    from longbow_amd import ivfsq8
    X, Q, C_, mn, mx, lists, codes = parity
    rng = np.random.default_rng(7)
    ids = rng.permutation(1 << 20)[:X.shape[0]].astype(np.int64) + (np.arange(X.shape[0], dtype=np.int64) % 3 << 41)
    one = _handle(X, C_, mn, mx, ids=ids)
    pieces = _handle(X[:0], C_, mn, mx)
    dev = _handle(X[:0], C_, mn, mx)
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
        _check_search(oracle, pieces, 0, Q[:5], C_, lists[:r0], codes[:r0], mn, mx, 10, 3, ids=ids, ctx=f"after {r0} rows")
    assert r0 == X.shape[0]
    want = one.search(Q, 10, 3)
    ol, od, _ = sqo.search(oracle, 0, Q, C_, lists, codes, mn, mx, 10, 3, ids=ids)
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
    for h, bad in ((pieces, None), (_handle(X[:5], C_, mn, mx), ids[:3])):
        before = h.ntotal
        rc = h._lib.lb_gpu_ivfsq8_add(h._h, 3, X.ctypes.data, bad.ctypes.data if bad is not None else None)
        assert rc == INVALID and h.ntotal == before
        with pytest.raises(ivfsq8._lib.LongbowGPUError, match="ids"):
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


@pytest.mark.parametrize("order", [0, 1])
def test_the_partition_is_the_ivf_flat_handle_s(oracle, parity, order):
    """the same centroids and rows, added in three pieces with ids: both handles hold the partition the oracle assigns"""
    from longbow_amd import ivf
    X, Q, C_, mn, mx, lists, _ = parity
    if order:
        lists = sqo.assign(oracle, order, X, C_)
    ids = np.random.default_rng(12).permutation(1 << 20)[:X.shape[0]].astype(np.int64) + (1 << 41)
    codes_h = _handle(X[:0], C_, mn, mx, order)
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
def test_batches_concurrent_and_profiled_searches(oracle, parity):
    """1025 queries run as two batches.  A profiled search records an event between the steps of each and drains after each: it
    returns what the unprofiled search returns, and the five slots (probes, plan, codes, scan, select) sum over the batches."""
    X, Q, C_, mn, mx, lists, codes = parity
    big = np.random.default_rng(8).standard_normal((1025, X.shape[1])).astype(F)
    h = _handle(X, C_, mn, mx)
    ol, od, scanned = sqo.search(oracle, 0, big, C_, lists, codes, mn, mx, 10, 3)
    for nq in (1, 1025):
        lab, dist = h.search(big[:nq], 10, 3)
        assert_same(lab, dist, ol[:nq], od[:nq], f"nq {nq}")
        assert h.last_search_stats()[:2] == (nq, int(scanned[:nq].sum()))
    stats = h.last_search_stats()
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
    assert h.last_timing() == (0.0,) * 5
    h.set_profiling(True)
    assert_same(*h.search(big, 10, 3), ol, od, "profiled against unprofiled")
    assert h.last_search_stats() == stats
    ms = h.last_timing()
    assert len(ms) == 5 and all(np.isfinite(t) and t >= 0 for t in ms) and sum(ms) > 0, ms
    h.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_every_list_probed_without_the_coarse_search(oracle):
    """2100 lists are more than the LB_MAX_K probes the coarse search returns: with all of them probed the probes are the lists"""
    X, Q, C_, mn, mx = sqo.parity_case(16, n=5000, nlist=2100, nq=5)
    lists, codes = sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)
    h = _handle(X, C_, mn, mx)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.list_sizes(), np.bincount(lists, minlength=2100))
    bl, bd = sqo.brute(Q, codes, mn, mx, 10)
    for nprobe in (2100, 5000):
        lab, dist = h.search(Q, 10, nprobe)
        assert_same(lab, dist, bl, bd, f"nprobe {nprobe}")
        assert h.last_search_stats() == (5, 5 * 5000, 5000, 5)
    _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, 10, 40, ctx="nprobe 40 of 2100")
    dist = np.full((5, 10), 9.0, F)
    lab = np.full((5, 10), 77, np.int64)
    assert h._lib.lb_gpu_ivfsq8_search(h._h, 5, Q.ctypes.data, 10, 2099, dist.ctypes.data, lab.ctypes.data) == UNSUPPORTED
    assert (dist == 9.0).all() and (lab == 77).all()
    h.Close()


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_refusals_behind_a_live_handle(oracle, parity):
    from longbow_amd import gpu
    X, Q, C_, mn, mx, lists, codes = parity
    h = _handle(X, C_, mn, mx)
    lib = h._lib
    kmax = LB_MAX_K + 1
    dist = np.full((Q.shape[0], kmax), 9.0, F)
    lab = np.full((Q.shape[0], kmax), 77, np.int64)
    u8 = np.full(2 * X.shape[1], 0xA5, np.uint8)
    args = (Q.shape[0], Q.ctypes.data)
    assert lib.lb_gpu_ivfsq8_search(h._h, *args, kmax, 3, dist.ctypes.data, lab.ctypes.data) == UNSUPPORTED
    assert b"2048" in lib.lb_gpu_ivfsq8_last_error(h._h)
    assert lib.lb_gpu_ivfsq8_search(h._h, *args, 10, 0, dist.ctypes.data, lab.ctypes.data) == INVALID
    assert b"nprobe" in lib.lb_gpu_ivfsq8_last_error(h._h)
    assert lib.lb_gpu_ivfsq8_search(h._h, *args, 10, -4, dist.ctypes.data, lab.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfsq8_search(h._h, *args, 0, 3, dist.ctypes.data, lab.ctypes.data) == INVALID
    c = gpu.Cancel()
    c.fire()
    assert lib.lb_gpu_ivfsq8_search_ctx(h._h, *args, 10, 3, dist.ctypes.data, lab.ctypes.data, c._h) == CANCELLED
    assert lib.lb_gpu_ivfsq8_assignments(h._h, X.shape[0] - 1, 2, lab.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfsq8_get_codes(h._h, X.shape[0] - 1, 2, u8.ctypes.data) == INVALID
    assert (dist == 9.0).all() and (lab == 77).all() and (u8 == 0xA5).all()
    st = (C.c_int64 * 4)()
    assert lib.lb_gpu_ivfsq8_last_search_stats(h._h, st) == 0
    # a query with a NaN component: its code is 0 there, and the coarse search ranks the NaN distances last, by position
    Qn = Q[:6].copy()
    Qn[1, 3] = np.nan
    Qn[4] = np.nan
    assert so.encode(Qn, mn, mx)[1, 3] == 0 and not so.encode(Qn, mn, mx)[4].any()
    for nprobe in (3, 16):
        _check_search(oracle, h, 0, Qn, C_, lists, codes, mn, mx, 10, nprobe, ctx=f"NaN queries nprobe {nprobe}")
    # the codes once, lists, assignments: what a row costs, plus the centroids
    n = X.shape[0]
    assert h.hbm_bytes >= n * (X.shape[1] + 12) + C_.nbytes
    h.Close()
    e = _handle(X[:0], C_, mn, mx)  # nothing stored: all padding
    el, ed = e.search(Q, 7, 2)
    assert (el == -1).all() and (ed == sqo.FLT_MAX).all() and e.last_search_stats() == (Q.shape[0], 0, 0, 0)
    assert e.codes().shape == (0, X.shape[1]) and e.list_sizes().sum() == 0
    e.Close()


# 12 --------------------------------------------------------------------------------------------------------------------------
def _check_filtered(oracle, h, Q, C_, lists, codes, mn, mx, mask, k, nprobe, ids=None, ctx=""):
    assert h.nvisible() == np.count_nonzero(mask), ctx
    return _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, k, nprobe, ids=ids, mask=mask, ctx=ctx)


def test_row_filter_masks(oracle, parity):
    from longbow_amd import _lib
    X, Q, C_, mn, mx, lists, codes = parity
    n = X.shape[0]
    rng = np.random.default_rng(17)
    one_per_list = np.zeros(n, np.uint8)
    for l in range(C_.shape[0]):
        rows = np.flatnonzero(lists == l)
        if rows.size:
            one_per_list[rows[rows.size // 2]] = 0x80
    masks = {"all visible": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "10 % byte mask": rv.byte_mask(rng, n, 0.1),
             "one row per list": one_per_list}
    h, twin = _handle(X, C_, mn, mx), _handle(X, C_, mn, mx)
    enc = _sq8_handle(mn, mx, codes)
    for name, mask in masks.items():
        h.set_filter(mask)
        assert h.ntotal == n
        for nprobe in (1, 3, 16):
            _check_filtered(oracle, h, Q, C_, lists, codes, mn, mx, mask, 10, nprobe, ctx=f"{name}, nprobe {nprobe}")
        # every list probed equals the flat SQ8 handle under the same mask
        enc.set_filter(mask)
        assert_same(*h.search(Q, 10, 21), *enc.search(Q, 10), f"{name}, against the filtered SQ8 handle")
    # what addresses the lists themselves ignores the filter
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    assert np.array_equal(h.codes(), codes)
    # a wrong-length mask is refused and leaves the filter as it was
    mask = masks["10 % byte mask"]
    h.set_filter(mask)
    want = h.search(Q, 10, 3)
    for bad in (mask[:-1], np.concatenate([mask, mask[:1]])):
        with pytest.raises(_lib.LongbowGPUError) as e:
            h.set_filter(bad)
        assert e.value.code == INVALID and "rows" in str(e.value)
        assert h.nvisible() == np.count_nonzero(mask)
        assert_same(*h.search(Q, 10, 3), *want, "after a refused length")
    # clearing the filter restores the unfiltered result
    h.set_filter(None)
    assert h.nvisible() == h.ntotal == n
    for nprobe in (1, 3, 16):
        assert_same(*h.search(Q, 10, nprobe), *twin.search(Q, 10, nprobe), f"cleared, nprobe {nprobe}")
        assert h.last_search_stats() == twin.last_search_stats()
    for x in (h, twin, enc):
        x.Close()


def test_filter_column_and_combine(oracle, parity):
    X, Q, C_, mn, mx, lists, codes = parity
    n = X.shape[0]
    rng = np.random.default_rng(18)
    valid = rng.random(n) < 0.8
    icol, ival = rv.int64_edge_column(n), 2 ** 32
    fcol, fval = rv.float32_edge_column(n), 0.25
    h = _handle(X, C_, mn, mx)
    for voff in (0, 3):
        h.filter_column(icol, ival, rv.LT, valid=rv.validity_bitmap(valid, voff), validity_offset=voff)
        m1 = rv.predicate(icol, ival, rv.LT, valid)
        _check_filtered(oracle, h, Q, C_, lists, codes, mn, mx, m1, 10, 3, ctx=f"int64 LT, validity offset {voff}")
        h.filter_column(fcol, fval, rv.GE, valid=rv.validity_bitmap(valid, voff), validity_offset=voff)
        _check_filtered(oracle, h, Q, C_, lists, codes, mn, mx, rv.predicate(fcol, fval, rv.GE, valid), 10, 3,
                        ctx=f"float32 GE, validity offset {voff}")
    h.filter_column(icol, ival, rv.LT, valid=rv.validity_bitmap(valid, 3), validity_offset=3)
    h.filter_column(fcol, fval, rv.LE, combine=True)
    m2 = rv.and_bytes(m1, rv.predicate(fcol, fval, rv.LE))
    assert 0 < m2.sum() < m1.sum()
    _check_filtered(oracle, h, Q, C_, lists, codes, mn, mx, m2, 10, 3, ctx="combine after a predicate")
    byte_mask = rv.byte_mask(rng, n, 0.5)
    h.set_filter(byte_mask)
    h.filter_column(icol, ival, rv.LT, combine=True)
    m3 = rv.and_bytes(byte_mask, rv.predicate(icol, ival, rv.LT))
    assert 0 < np.count_nonzero(m3) < np.count_nonzero(byte_mask)
    _check_filtered(oracle, h, Q, C_, lists, codes, mn, mx, m3, 10, 3, ctx="combine after a byte mask")
    h.Close()


@pytest.mark.parametrize("with_ids", [False, True])
def test_adds_under_a_filter(oracle, parity, with_ids):
    """1000 rows, a 50 % mask, then two more adds with reserve never called: the second takes the handle past its 4096-row
    buffers under the active filter"""
    X, Q, C_, mn, mx, lists, codes = parity
    rng = np.random.default_rng(7)
    more = rng.standard_normal((2000, X.shape[1])).astype(F)
    all_rows = np.concatenate([X, more])
    all_lists = np.concatenate([lists, sqo.assign(oracle, 0, more, C_)])
    all_codes = sqo.encode(all_rows, mn, mx)
    ids = rng.permutation(1 << 20)[:all_rows.shape[0]].astype(np.int64) + (1 << 41) if with_ids else None
    sub = lambda a, b: None if ids is None else ids[a:b]
    mask = rv.byte_mask(rng, 1000, 0.5)
    h = _handle(X[:1000], C_, mn, mx, ids=sub(0, 1000))
    h.set_filter(mask)
    for n in (3000, 5000):
        h.add(all_rows[h.ntotal:n], sub(h.ntotal, n))
        full = np.concatenate([mask, np.ones(n - 1000, np.uint8)])
        assert h.ntotal == n and np.array_equal(h.assignments(), all_lists[:n]) and np.array_equal(h.codes(), all_codes[:n])
        for nprobe in (3, 16):
            _check_filtered(oracle, h, Q, C_, all_lists[:n], all_codes[:n], mn, mx, full, 10, nprobe, ids=sub(0, n),
                            ctx=f"{n} rows nprobe {nprobe}")
    h.Close()


# 13 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True])
def test_search_refine(oracle, parity, f16):
    from longbow_amd import gpu
    X, Q, C_, mn, mx, lists, codes = parity
    rows = X.astype(np.float16) if f16 else X
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=X.shape[1], Metric=0,
                                               DataType=gpu.DataType.Float16 if f16 else gpu.DataType.Float32))
    h = _handle(X, C_, mn, mx)
    with_ids = _handle(X[:50], C_, mn, mx, ids=np.arange(50, dtype=np.int64) + 10 ** 6)
    try:
        idx.Add(None, rows)
        short, _, _ = sqo.search(oracle, 0, Q, C_, lists, codes, mn, mx, 64, 2)  # the oracle's shortlist
        for order in (0, 1):
            lab, dist = h.search_refine(idx, Q, 5, 64, 2, order=order)
            assert_same(lab, dist, *fo.refine(oracle, 0, Q, rows.astype(F), short, 5, order), f"f16 {f16} order {order}")
        with pytest.raises(ValueError):
            with_ids.search_refine(idx, Q, 5, 64, 2)
    finally:
        idx.Close()
        h.Close()
        with_ids.Close()


def test_python_front_end(parity):
    from longbow_amd import ivfsq8, sq8
    X, Q, C_, mn, mx, lists, codes = parity
    with pytest.raises(ValueError, match="min must be less than max"):
        ivfsq8.IVFSQ8(mn, mn, C_)
    cent, tmn, tmx = ivfsq8.train(X[:1500], 8, max_iter=2, seed=3)
    assert cent.shape == (8, X.shape[1]) and np.array_equal(tmn, so.train(X[:1500])[0]) and np.array_equal(tmx, so.train(X[:1500])[1])
    t = ivfsq8.IVFSQ8(tmn, tmx, cent)
    t.add(X[:1500])
    enc = sq8.SQ8Encoder(X.shape[1])
    enc.set_bounds(tmn, tmx)
    assert np.array_equal(t.codes(), enc.Encode(X[:1500]))
    enc.add_codes(t.codes())
    assert_same(*t.search(Q, 5, 8), *enc.search(Q, 5), "trained, every list probed")
    enc.Close()
    t.Close()


# the shared add across two pieces (tests/ivf_piece_cases.py) ----------------------------------------------------------------
@pytest.fixture(scope="module")
def two_pieces(oracle):
    """the case, a maker of empty handles over it, the snapshot of one filled by small adds and the oracle's assignment"""
    gpu_or_skip()
    X, ids, C_, Q = pc.case()
    mn, mx = X.min(axis=0), X.max(axis=0)
    new = lambda: _handle(X[:0], C_, mn, mx)
    return X, ids, Q, new, pc.reference(new, X, ids, Q), sqo.assign(oracle, 0, X, C_)


@pytest.mark.parametrize("device", [False, True])
def test_one_add_across_pieces(two_pieces, device):
    X, ids, Q, new, want, lists = two_pieces
    pc.check_one_add(new, X, ids, Q, want, lists, device)


def test_one_add_across_pieces_under_a_filter_and_removals(two_pieces):
    """the add's tail is the shared one whatever the pieces: onto 300 rows under a filter that hides a third of them, three rows
    removed, the one add of two pieces leaves what adds of single pieces leave"""
    X, ids, Q, new, _, _ = two_pieces
    first = ids[:300] + 1  # (ids of their own: those of the case are multiples of 3 above 2^40)
    mask = (np.arange(300) % 3 != 0).astype(np.uint8)

    def run(step):
        h = new()
        h.add(X[:300], first)
        h.set_filter(mask)
        assert h.remove(first[[4, 100, 299]]) == 3  # (rows the filter shows)
        pc.fill(h, X, ids, step)
        out = (h.ntotal, h.nvisible(), h.nlive(), h.ndeleted(), h.list_sizes(), *h.search(Q, pc.K, pc.NPROBE))
        h.Close()
        return out

    got, want = run(pc.N), run(pc.SMALL)
    assert got[:4] == want[:4] == (300 + pc.N, 200 - 3 + pc.N, 300 - 3 + pc.N, 3), (got[:4], want[:4])
    assert np.array_equal(got[4], want[4])
    assert_same(got[5], got[6], want[5], want[6], "one add against single pieces")
    hidden = np.concatenate((first[::3], first[[4, 100, 299]]))
    assert (got[5] >= 0).all() and not np.isin(got[5], hidden).any()
