"""lb_gpu_ivfbq_* on the GPU against tests/ivfbq_oracle.py (the semantics restated over tests/ivf_oracle.py's lists and probes and
tests/bq_oracle.py's encode, hamming and topk): labels and distances must be equal, bit for bit.  The shapes are the smallest at
which the kernels can still go wrong: one word and two words with pad bits, the workload's 12-word chunk, the 16-word boundary
and 17 words in three chunks; lists around the 256-row tile, a list whose workgroups take a second tile, list boundaries inside
a wave; selections within LDS and beyond it; ties across lists; more queries than a batch."""
import threading

import numpy as np
import pytest

from tests import bq_oracle as bo
from tests import ivfbq_oracle as bqo
from tests import ivf_piece_cases as pc
from tests import refine_oracle as fo
from tests import row_view_cases as rv
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED, CANCELLED = 1, 6, 8
LB_MAX_K = 2048
LDS_KEYS = bqo.LDS_KEYS


def _handle(X, C_, order=0, ids=None):
    from longbow_amd import ivfbq
    gpu_or_skip()
    h = ivfbq.IVFBQ(C_, order)
    if X.shape[0]:
        h.add(X, ids)
    return h


def _check_search(oracle, h, order, Q, C_, lists, codes, k, nprobe, ids=None, mask=None, ctx=""):
    ol, od, scanned = bqo.search(oracle, order, Q, C_, lists, codes, k, nprobe, ids=ids, mask=mask)
    lab, dist = h.search(Q, k, nprobe)
    assert_same(lab, dist, ol, od, ctx)
    st = h.last_search_stats()
    assert st[0] == Q.shape[0] and st[1] == int(scanned.sum()) and st[2] == int(scanned.max()), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= LDS_KEYS).sum()), (st, ctx)
    return scanned


def _bq_handle(dims, codes):
    from longbow_amd import bq
    enc = bq.BQEncoder(dims)
    enc.add_codes(codes)
    return enc


@pytest.fixture(scope="module")
def parity(oracle):
    """the two-word shape of case 1 with its oracle lists and codes at order 0 (shared by the adds, batches, refusals, filters,
    the refine and the threads)"""
    X, Q, C_ = bqo.parity_case(100)
    return X, Q, C_, bqo.assign(oracle, 0, X, C_), bqo.encode(X)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dims", bqo.PARITY_DIMS)
def test_parity_grid(oracle, dims, order):
    X, Q, C_ = bqo.parity_case(dims)
    lists, codes = bqo.assign(oracle, order, X, C_), bqo.encode(X)
    h = _handle(X, C_, order)
    assert h.ntotal == X.shape[0] and (h.nlist, h.dims) == C_.shape and h.order == order and h.words == bo.words(dims)
    assert h._lib.lb_gpu_ivfbq_dims(h._h) == dims and h._lib.lb_gpu_ivfbq_order(h._h) == order and h._lib.lb_gpu_ivfbq_nlist(h._h) == 16
    assert np.array_equal(h.assignments(), lists)
    assert np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    assert np.array_equal(h.codes(), codes) and np.array_equal(h.codes(100, 7), codes[100:107])
    assert np.array_equal(h.centroids(), C_)
    for nprobe in (1, 3, 16):
        _check_search(oracle, h, order, Q, C_, lists, codes, 10, nprobe, ctx=f"dims {dims} order {order} nprobe {nprobe}")
    h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [16, 768])
def test_every_list_probed_equals_the_bq_handle(dims):
    X, Q, C_ = bqo.parity_case(dims)
    n = X.shape[0]
    ids = np.random.default_rng(2).permutation(1 << 22)[:n].astype(np.int64) + (1 << 41)
    for with_ids in (False, True):
        h = _handle(X, C_, ids=ids if with_ids else None)
        enc = _bq_handle(dims, h.codes())
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
def test_ties_come_in_row_order(oracle):
    """tests/test_ivfbq_semantics.py asserts of this input that every query's top 10 holds a tie group whose rows lie in more
    than one list"""
    X3, Q, C_ = bqo.tie_case()
    n = X3.shape[0] // 3
    lists3, codes3 = np.tile(bqo.assign(oracle, 0, X3[:n], C_), 3), bqo.encode(X3)
    h = _handle(X3, C_)
    assert np.array_equal(h.codes(), codes3) and np.array_equal(h.assignments(), lists3)
    for nprobe in (2, 16):
        _check_search(oracle, h, 0, Q, C_, lists3, codes3, 10, nprobe, ctx=f"ties nprobe {nprobe}")
    lab, dist = h.search(Q, 10, 16)
    tie = dist[:, 1:] == dist[:, :-1]
    assert (tie.sum(axis=1) >= 2).all() and (lab[:, 1:][tie] > lab[:, :-1][tie]).all()
    assert (dist == np.floor(dist)).all() and (dist >= 0).all() and (dist <= 16).all()
    h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_list_length_edges(oracle):
    """tests/test_ivfbq_semantics.py asserts of this input what the case needs: the counts, a workgroup's second tile at
    nprobe = 1 and several list boundaries inside one wave with every list probed"""
    X, Q, C_, owner = bqo.edge_case()
    codes = bqo.encode(X)
    h = _handle(X, C_)
    assert np.array_equal(h.assignments(), owner) and h.list_sizes().tolist() == list(bqo.EDGE_COUNTS)
    assert np.array_equal(h.codes(), codes)
    nlist = C_.shape[0]
    for nprobe, k in ((1, 10), (1, 300), (2, 10), (5, 300), (nlist, 10), (nlist, 300)):
        _check_search(oracle, h, 0, Q, C_, owner, codes, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
    lab, dist = h.search(Q, 10, 1)
    assert (lab[0] == -1).all() and (dist[0] == bqo.FLT_MAX).all()  # an empty probed list: all padding
    assert lab[1, 0] == np.flatnonzero(owner == 1)[0] and (lab[1, 1:] == -1).all() and (dist[1, 1:] == bqo.FLT_MAX).all()  # P_q < k
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_the_long_selection(oracle):
    X, Q, C_ = bqo.skew_case()
    lists, codes = bqo.assign(oracle, 0, X, C_), bqo.encode(X)
    h = _handle(X, C_)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.codes(), codes)
    from_lds = []
    for nprobe in (1, 4):
        for k in (1, 100, 2048):
            scanned = _check_search(oracle, h, 0, Q, C_, lists, codes, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
            from_lds.append(h.last_search_stats()[3])
    assert scanned.min() > LDS_KEYS
    # nprobe = 1: three queries scan list 0 (beyond LDS), two scan list 2 (within); nprobe = 4: all scan both lists
    assert from_lds == [2, 2, 2, 0, 0, 0]
    h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_batches_limits_and_refusals(oracle, parity):
    from longbow_amd import gpu
    X, Q, C_, lists, codes = parity
    big = np.random.default_rng(8).standard_normal((1030, X.shape[1])).astype(F)
    h = _handle(X, C_)
    lib = h._lib
    ol, od, scanned = bqo.search(oracle, 0, big, C_, lists, codes, 10, 3)
    for nq in (1, 1030):  # 1030 queries run as two batches
        lab, dist = h.search(big[:nq], 10, 3)
        assert_same(lab, dist, ol[:nq], od[:nq], f"nq {nq}")
        assert h.last_search_stats()[:2] == (nq, int(scanned[:nq].sum()))
    # a profiled search returns what the unprofiled one returns, and the five slots sum over the batches
    stats = h.last_search_stats()
    assert h.last_timing() == (0.0,) * 5
    h.set_profiling(True)
    assert_same(*h.search(big, 10, 3), ol, od, "profiled against unprofiled")
    assert h.last_search_stats() == stats
    ms = h.last_timing()
    assert len(ms) == 5 and all(np.isfinite(t) and t >= 0 for t in ms) and sum(ms) > 0, ms
    h.set_profiling(False)
    # k = LB_MAX_K, and P_q < k gives padding
    _check_search(oracle, h, 0, Q[:4], C_, lists, codes, LB_MAX_K, 16, ctx="k = LB_MAX_K, every list")
    _check_search(oracle, h, 0, Q[:4], C_, lists, codes, LB_MAX_K, 2, ctx="k = LB_MAX_K, two lists")
    stats = h.last_search_stats()
    kmax = LB_MAX_K + 1
    dist = np.full((Q.shape[0], kmax), 9.0, F)
    lab = np.full((Q.shape[0], kmax), 77, np.int64)
    u64 = np.full(2 * h.words, 0xA5A5A5A5A5A5A5A5, np.uint64)
    args = (Q.shape[0], Q.ctypes.data)
    assert lib.lb_gpu_ivfbq_search(h._h, *args, kmax, 3, dist.ctypes.data, lab.ctypes.data) == UNSUPPORTED
    assert b"2048" in lib.lb_gpu_ivfbq_last_error(h._h)
    assert lib.lb_gpu_ivfbq_search(h._h, *args, 10, 0, dist.ctypes.data, lab.ctypes.data) == INVALID
    assert b"nprobe" in lib.lb_gpu_ivfbq_last_error(h._h)
    assert lib.lb_gpu_ivfbq_search(h._h, *args, 10, -4, dist.ctypes.data, lab.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfbq_search(h._h, *args, 0, 3, dist.ctypes.data, lab.ctypes.data) == INVALID
    c = gpu.Cancel()
    c.fire()
    assert lib.lb_gpu_ivfbq_search_ctx(h._h, *args, 10, 3, dist.ctypes.data, lab.ctypes.data, c._h) == CANCELLED
    assert lib.lb_gpu_ivfbq_assignments(h._h, X.shape[0] - 1, 2, lab.ctypes.data) == INVALID
    assert lib.lb_gpu_ivfbq_get_codes(h._h, X.shape[0] - 1, 2, u64.ctypes.data) == INVALID
    assert (dist == 9.0).all() and (lab == 77).all() and (u64 == 0xA5A5A5A5A5A5A5A5).all()
    assert h.last_search_stats() == stats  # a refused or cancelled search publishes none
    # a query with a NaN component: its bit is 0 there, and the coarse search ranks the NaN distances last, by position
    Qn = Q[:6].copy()
    Qn[1, 3] = np.nan
    Qn[4] = np.nan
    assert not (int(bo.encode(Qn)[1, 0]) >> 3) & 1 and not bo.encode(Qn)[4].any()
    for nprobe in (3, 16):
        _check_search(oracle, h, 0, Qn, C_, lists, codes, 10, nprobe, ctx=f"NaN queries nprobe {nprobe}")
    # the codes three times, lists, assignments: what a row costs, plus the centroids
    n = X.shape[0]
    assert h.hbm_bytes >= n * (24 * h.words + 12) + C_.nbytes
    h.Close()
    e = _handle(X[:0], C_)  # nothing stored: all padding
    el, ed = e.search(Q, 7, 2)
    assert (el == -1).all() and (ed == bqo.FLT_MAX).all() and e.last_search_stats() == (Q.shape[0], 0, 0, 0)
    assert e.codes().shape == (0, 2) and e.list_sizes().sum() == 0
    e.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_adds_in_pieces_with_ids(oracle, parity):
    import torch
    from longbow_amd import ivfbq
    X, Q, C_, lists, codes = parity
    rng = np.random.default_rng(7)
    ids = rng.permutation(1 << 20)[:X.shape[0]].astype(np.int64) + (np.arange(X.shape[0], dtype=np.int64) % 3 << 41)
    one = _handle(X, C_, ids=ids)
    pieces = _handle(X[:0], C_)
    dev = _handle(X[:0], C_)
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
        _check_search(oracle, pieces, 0, Q[:5], C_, lists[:r0], codes[:r0], 10, 3, ids=ids, ctx=f"after {r0} rows")
    assert r0 == X.shape[0]
    want = one.search(Q, 10, 3)
    ol, od, _ = bqo.search(oracle, 0, Q, C_, lists, codes, 10, 3, ids=ids)
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
    for h, bad in ((pieces, None), (_handle(X[:5], C_), ids[:3])):
        before = h.ntotal
        rc = h._lib.lb_gpu_ivfbq_add(h._h, 3, X.ctypes.data, bad.ctypes.data if bad is not None else None)
        assert rc == INVALID and h.ntotal == before
        with pytest.raises(ivfbq._lib.LongbowGPUError, match="ids"):
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
def _check_filtered(oracle, h, Q, C_, lists, codes, mask, k, nprobe, ids=None, ctx="", enc=None):
    """against the oracle under the mask; with enc (a bq.BQEncoder over the same codes) also every list probed against its
    search under the same mask"""
    assert h.nvisible() == np.count_nonzero(mask), ctx
    scanned = _check_search(oracle, h, 0, Q, C_, lists, codes, k, nprobe, ids=ids, mask=mask, ctx=ctx)
    if enc is not None:
        enc.set_filter(mask)
        fl, fd = enc.search(Q, k)
        if ids is not None:
            fl = np.where(fl >= 0, ids[np.clip(fl, 0, None)], -1)
        assert_same(*h.search(Q, k, C_.shape[0] + 5), fl, fd, ctx + ", against the filtered BQ handle")
        assert h.last_search_stats()[1] == Q.shape[0] * np.count_nonzero(mask), ctx
    return scanned


def test_row_filter_masks(oracle, parity):
    from longbow_amd import _lib
    X, Q, C_, lists, codes = parity
    n = X.shape[0]
    rng = np.random.default_rng(17)
    big_list = int(np.argmax(np.bincount(lists, minlength=C_.shape[0])))
    one_list_hidden = np.where(lists == big_list, 0, 0x80).astype(np.uint8)
    masks = {"all visible": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "10 % byte mask": rv.byte_mask(rng, n, 0.1),
             "one list wholly invisible": one_list_hidden}
    h, twin = _handle(X, C_), _handle(X, C_)
    enc = _bq_handle(X.shape[1], codes)
    for name, mask in masks.items():
        h.set_filter(mask)
        assert h.ntotal == n
        for nprobe in (1, 3, 16):
            _check_filtered(oracle, h, Q, C_, lists, codes, mask, 10, nprobe, ctx=f"{name}, nprobe {nprobe}", enc=enc)
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


@pytest.mark.parametrize("dims", [768, 1088])
def test_row_filter_on_wide_rows(oracle, dims):
    """the visible scan's gathers at the workload's single chunk and at three chunks"""
    X, Q, C_ = bqo.parity_case(dims)
    lists, codes = bqo.assign(oracle, 0, X, C_), bqo.encode(X)
    mask = rv.byte_mask(np.random.default_rng(19), X.shape[0], 0.3)
    h = _handle(X, C_)
    h.set_filter(mask)
    for nprobe in (3, 16):
        _check_filtered(oracle, h, Q, C_, lists, codes, mask, 10, nprobe, ctx=f"dims {dims} nprobe {nprobe}")
    h.Close()


@pytest.mark.parametrize("filtered", [False, True])
def test_one_workgroup_walks_several_tiles_and_chunks(oracle, filtered):
    """1024 queries x 4 probes = 4,096 pairs, so the scan's grid has one workgroup per (query, list): it walks the three or more
    256-row tiles of the longest list, the last one partial, in three chunks each (1088 dims: 17 words, 8 + 8 + 1), and the
    pipeline wraps from a tile's last chunk to the next tile's first.  Without a filter, and with every third row hidden (the scan
    of the visible lists)"""
    nq, nprobe, dims, n = 1024, 4, 1088, 6000
    X, Q, C_ = bqo.parity_case(dims, n=n, nlist=8, nq=nq)
    lists, codes = bqo.assign(oracle, 0, X, C_), bqo.encode(X)
    mask = (np.arange(n) % 3 != 0).astype(np.uint8) if filtered else None
    big = int(np.bincount(lists if mask is None else lists[mask != 0], minlength=8).max())
    W = bo.words(dims)
    assert bqo.scan_tiles_x(nq * nprobe, big) == 1
    assert big > 2 * bqo.TILE and big % bqo.TILE != 0, big
    assert bqo.chunks(W) >= 2 and W % bqo.chunk_words(W) != 0
    h = _handle(X, C_)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.codes(), codes)
    if filtered:
        h.set_filter(mask)
        assert h.nvisible() == np.count_nonzero(mask)
    _check_search(oracle, h, 0, Q, C_, lists, codes, 10, nprobe, mask=mask, ctx=f"several tiles and chunks, filtered {filtered}")
    h.Close()


def test_filter_column_and_combine(oracle, parity):
    X, Q, C_, lists, codes = parity
    n = X.shape[0]
    rng = np.random.default_rng(18)
    valid = rng.random(n) < 0.8
    icol, ival = rv.int64_edge_column(n), 2 ** 32
    fcol, fval = rv.float32_edge_column(n), 0.25
    h = _handle(X, C_)
    enc = _bq_handle(X.shape[1], codes)
    for voff in (0, 3):
        h.filter_column(icol, ival, rv.LT, valid=rv.validity_bitmap(valid, voff), validity_offset=voff)
        m1 = rv.predicate(icol, ival, rv.LT, valid)
        _check_filtered(oracle, h, Q, C_, lists, codes, m1, 10, 3, ctx=f"int64 LT, validity offset {voff}", enc=enc)
        h.filter_column(fcol, fval, rv.GE, valid=rv.validity_bitmap(valid, voff), validity_offset=voff)
        _check_filtered(oracle, h, Q, C_, lists, codes, rv.predicate(fcol, fval, rv.GE, valid), 10, 3,
                        ctx=f"float32 GE, validity offset {voff}", enc=enc)
    h.filter_column(icol, ival, rv.LT, valid=rv.validity_bitmap(valid, 3), validity_offset=3)
    h.filter_column(fcol, fval, rv.LE, combine=True)
    m2 = rv.and_bytes(m1, rv.predicate(fcol, fval, rv.LE))
    assert 0 < m2.sum() < m1.sum()
    _check_filtered(oracle, h, Q, C_, lists, codes, m2, 10, 3, ctx="combine after a predicate", enc=enc)
    byte_mask = rv.byte_mask(rng, n, 0.5)
    h.set_filter(byte_mask)
    h.filter_column(icol, ival, rv.LT, combine=True)
    m3 = rv.and_bytes(byte_mask, rv.predicate(icol, ival, rv.LT))
    assert 0 < np.count_nonzero(m3) < np.count_nonzero(byte_mask)
    _check_filtered(oracle, h, Q, C_, lists, codes, m3, 10, 3, ctx="combine after a byte mask", enc=enc)
    enc.Close()
    h.Close()


@pytest.mark.parametrize("with_ids", [False, True])
def test_adds_under_a_filter(oracle, parity, with_ids):
    """1000 rows, a 50 % mask, then two more adds with reserve never called: the second takes the handle past its 4096-row
    buffers under the active filter"""
    X, Q, C_, lists, codes = parity
    rng = np.random.default_rng(7)
    more = rng.standard_normal((2000, X.shape[1])).astype(F)
    all_rows = np.concatenate([X, more])
    all_lists = np.concatenate([lists, bqo.assign(oracle, 0, more, C_)])
    all_codes = bqo.encode(all_rows)
    ids = rng.permutation(1 << 20)[:all_rows.shape[0]].astype(np.int64) + (1 << 41) if with_ids else None
    sub = lambda a, b: None if ids is None else ids[a:b]
    mask = rv.byte_mask(rng, 1000, 0.5)
    h = _handle(X[:1000], C_, ids=sub(0, 1000))
    h.set_filter(mask)
    for n in (3000, 5000):
        h.add(all_rows[h.ntotal:n], sub(h.ntotal, n))
        full = np.concatenate([mask, np.ones(n - 1000, np.uint8)])
        assert h.ntotal == n and np.array_equal(h.assignments(), all_lists[:n]) and np.array_equal(h.codes(), all_codes[:n])
        enc = _bq_handle(X.shape[1], all_codes[:n])
        for nprobe in (3, 16):
            _check_filtered(oracle, h, Q, C_, all_lists[:n], all_codes[:n], full, 10, nprobe, ids=sub(0, n),
                            ctx=f"{n} rows nprobe {nprobe}", enc=enc if nprobe == 16 else None)
        enc.Close()
    h.Close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_search_refine(oracle, parity):
    from longbow_amd import gpu
    X, Q, C_, lists, codes = parity
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=X.shape[1], Metric=0, DataType=gpu.DataType.Float32))
    h = _handle(X, C_)
    with_ids = _handle(X[:50], C_, ids=np.arange(50, dtype=np.int64) + 10 ** 6)
    try:
        idx.Add(None, X)
        short, _, _ = bqo.search(oracle, 0, Q, C_, lists, codes, 64, 2)  # the oracle's shortlist
        for order in (0, 1):
            lab, dist = h.search_refine(idx, Q, 5, 64, 2, order=order)
            assert_same(lab, dist, *fo.refine(oracle, 0, Q, X, short, 5, order), f"order {order}")
        with pytest.raises(ValueError):
            with_ids.search_refine(idx, Q, 5, 64, 2)
    finally:
        idx.Close()
        h.Close()
        with_ids.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_eight_threads_share_a_handle(oracle, parity):
    X, Q, C_, lists, codes = parity
    big = np.random.default_rng(9).standard_normal((8 * 40 + 160, X.shape[1])).astype(F)
    h = _handle(X, C_)
    ol, od = h.search(big, 10, 3)  # the single-threaded result, itself checked against the oracle on its first rows
    wl, wd, _ = bqo.search(oracle, 0, big[:40], C_, lists, codes, 10, 3)
    assert_same(ol[:40], od[:40], wl, wd, "single-threaded")
    out = [None] * 8

    def work(t):
        out[t] = h.search(big[t * 40:t * 40 + 200], 10, 3)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for t in range(8):
        assert_same(*out[t], ol[t * 40:t * 40 + 200], od[t * 40:t * 40 + 200], f"thread {t}")
    h.Close()


def test_python_front_end(parity):
    from longbow_amd import ivfbq
    X, Q, C_, lists, codes = parity
    cent = ivfbq.train(X[:1500], 8, max_iter=2, seed=3)
    assert cent.shape == (8, X.shape[1])
    t = ivfbq.IVFBQ(cent)
    t.add(X[:1500])
    assert np.array_equal(t.codes(), codes[:1500]) and t.words == 2
    enc = _bq_handle(X.shape[1], t.codes())
    assert_same(*t.search(Q, 5, 8), *enc.search(Q, 5), "trained, every list probed")
    enc.Close()
    t.Close()


# the shared add across two pieces (tests/ivf_piece_cases.py) ----------------------------------------------------------------
@pytest.fixture(scope="module")
def two_pieces(oracle):
    """the case, a maker of empty handles over it, the snapshot of one filled by small adds and the oracle's assignment"""
    gpu_or_skip()
    X, ids, C_, Q = pc.case()
    new = lambda: _handle(X[:0], C_)
    return X, ids, Q, new, pc.reference(new, X, ids, Q), bqo.assign(oracle, 0, X, C_)


@pytest.mark.parametrize("device", [False, True])
def test_one_add_across_pieces(two_pieces, device):
    X, ids, Q, new, want, lists = two_pieces
    pc.check_one_add(new, X, ids, Q, want, lists, device)
