"""Row filters on the IVF-PQ handle (lb_gpu_ivfpq_set_filter, _filter_int64 / _float32, _nvisible) on the GPU.  The expected result
everywhere is tests/ivfpq_filter_cases.py's search_filtered (the IVF-PQ oracle over the lists with the hidden rows taken out,
pinned on the CPU by tests/test_ivfpq_filter_semantics.py together with the keeps below); labels and distances are compared for
equality, and lb_gpu_ivfpq_last_search_stats shows that a search walked the visible rows alone.  The shapes are the smallest at
which the build of the visible lists (positions into the list-major codes) and the scan through them can go wrong: lists emptied
by the mask, visible lengths around the scan's 1024-position tile and beyond one step of its stride loop, the selection's 16,384
LDS keys, every form of the scan, a capacity that changes under an active filter, more lists than the coarse search returns."""
import threading

import numpy as np
import pytest

from tests import ivf_filter_cases as fc
from tests import ivfpq_filter_cases as pfc
from tests import ivfpq_oracle as pqo
from tests import row_view_cases as rv
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = 1
K = pfc.K


def _handle(X, C_, cb, order=0, ids=None):
    from longbow_amd import ivfpq
    gpu_or_skip()
    h = ivfpq.IVFPQ(pqo.blob(cb), C_, order)
    if X.shape[0]:
        h.add(X, ids)
    return h


def _check(oracle, h, cb, order, Q, C_, lists, codes, mask, k, nprobe, ids=None, ctx=""):
    """nvisible, labels, distances and the counters of a search under `mask` against the helper -> visible rows scanned"""
    ol, od, scanned = pfc.search_filtered(oracle, cb, order, Q, C_, lists, codes, mask, k, nprobe, ids=ids)
    assert h.nvisible() == np.count_nonzero(mask), ctx
    lab, dist = h.search(Q, k, nprobe)
    assert_same(lab, dist, ol, od, ctx)
    st = h.last_search_stats()
    assert st[:3] == (Q.shape[0], int(scanned.sum()), int(scanned.max())), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= pfc.LDS_KEYS).sum()), (st, ctx)
    return scanned


@pytest.fixture(scope="module")
def parity(oracle):
    """the byte-form shape with its oracle lists and codes at order 0"""
    X, Q, C_, cb = pqo.parity_case(*pqo.PARITY_SHAPES[0])
    return X, Q, C_, cb, pqo.assign(oracle, 0, X, C_), pqo.encode(oracle, cb, X)


@pytest.fixture(scope="module")
def edge(oracle):
    X, Q, C_, owner, cb = pqo.edge_case()
    return X, Q, C_, owner, cb, pqo.encode(oracle, cb, X)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dims,M", pqo.PARITY_SHAPES)
def test_parity_under_every_mask(oracle, dims, M, order):
    X, Q, C_, cb = pqo.parity_case(dims, M)
    lists, codes = pqo.assign(oracle, order, X, C_), pqo.encode(oracle, cb, X)
    h = _handle(X, C_, cb, order)
    masks = fc.parity_masks()
    names = list(masks) if ((dims, M), order) == (pqo.PARITY_SHAPES[0], 0) else ["10 % byte mask", "50 % byte mask"]
    for name in names:
        h.set_filter(masks[name])
        assert h.ntotal == X.shape[0]
        for nprobe in (1, 3, 16):
            _check(oracle, h, cb, order, Q, C_, lists, codes, masks[name], K, nprobe, ctx=f"{name}, dims {dims} M {M} order {order} nprobe {nprobe}")
    # what addresses the rows and the lists themselves ignores the filter
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    assert np.array_equal(h.codes(), codes) and np.array_equal(h.centroids(), C_)
    h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,M,n", [(16, 4, 3000), (32, 16, 70000)])
def test_every_list_probed_equals_the_filtered_pq_handle(dims, M, n):
    """70,000 rows: 35 compaction workgroups, and the PQ handle's list kernels with their sampled threshold and prefilter"""
    from longbow_amd import pq
    X, Q, C_, cb = pqo.parity_case(dims, M, n=n)
    rng = np.random.default_rng(2)
    ids = rng.permutation(1 << 22)[:n].astype(np.int64) + (1 << 41)
    mask = rv.byte_mask(rng, n, 0.10)
    for with_ids in (False, True):
        h = _handle(X, C_, cb, ids=ids if with_ids else None)
        h.set_filter(mask)
        enc = pq.PQEncoder(pqo.blob(cb))
        enc.add_codes(h.codes())
        enc.set_filter(mask)
        for prefilter in (True, False):
            enc.set_prefilter(prefilter)
            fl, fd = enc.Search(Q, K)
            if with_ids:
                fl = np.where(fl >= 0, ids[np.clip(fl, 0, None)], -1)
            for nprobe in (16, 21):
                lab, dist = h.search(Q, K, nprobe)
                assert_same(lab, dist, fl, fd, f"dims {dims} M {M} n {n} ids {with_ids} prefilter {prefilter} nprobe {nprobe}")
                assert h.last_search_stats()[1] == Q.shape[0] * np.count_nonzero(mask)
        enc.Close()
        h.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("choice", ["first rows", "random rows"])
@pytest.mark.parametrize("keep", [pfc.EDGE_KEEP_A, pfc.EDGE_KEEP_B], ids=["A", "B"])
def test_visible_list_lengths_at_the_tile_edges(oracle, edge, keep, choice):
    X, Q, C_, owner, cb, codes = edge
    nlist = C_.shape[0]
    mask = fc.keep_per_list(owner, keep, None if choice == "first rows" else np.random.default_rng(6))
    h = _handle(X, C_, cb)
    h.set_filter(mask)
    assert h.list_sizes().tolist() == list(pqo.EDGE_COUNTS)
    for nprobe in (1, 2, nlist):
        for k in (10, 200):
            scanned = _check(oracle, h, cb, 0, Q, C_, owner, codes, mask, k, nprobe, ctx=f"{choice} nprobe {nprobe} k {k}")
            if nprobe == 1:
                assert scanned.tolist() == list(keep) * 6
    lab, dist = h.search(Q, 10, 1)
    for l in np.flatnonzero(np.asarray(keep) == 0):  # a probed list with no visible row, emptied or empty: all padding
        assert (lab[l] == -1).all() and (dist[l] == pqo.FLT_MAX).all()
    one = keep.index(1)
    assert lab[one, 0] == np.flatnonzero((owner == one) & (mask != 0))[0] and (lab[one, 1:] == -1).all() and (dist[one, 1:] == pqo.FLT_MAX).all()
    h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_the_selection_follows_the_visible_count(oracle):
    """50,000 rows: 25 compaction workgroups.  List 0 holds about 37,000 rows, more than any selection from LDS takes; with
    exactly 16,384 of them visible the three queries that probe it are selected from LDS, with one more not."""
    X, Q, C_, cb = pqo.skew_case()
    lists, codes = pqo.assign(oracle, 0, X, C_), pqo.encode(oracle, cb, X)
    h = _handle(X, C_, cb)
    for keep0, from_lds in ((pfc.LDS_KEYS, 5), (pfc.LDS_KEYS + 1, 2)):
        mask = fc.skew_mask(lists, keep0)
        h.set_filter(mask)
        for k in (1, 100, 2048):
            _check(oracle, h, cb, 0, Q, C_, lists, codes, mask, k, 1, ctx=f"{keep0} visible in list 0, k {k}")
            assert h.last_search_stats()[3] == from_lds
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,M,n,nlist,nprobes", [
    (192, 96, 2000, 8, (2, 8)),      # the workload's table: six 16-byte loads a row
    (159, 159, 500, 130, (2, 129)),  # the largest table, single bytes; 129 probes' segments no longer fit beside it
    (80, 80, 700, 8, (3,)),          # M % 16 == 0 without a compile-time form
    (4, 1, 1000, 8, (2, 8)),
])
def test_scan_forms_under_a_filter(oracle, dims, M, n, nlist, nprobes):
    X, Q, C_, cb = pqo.parity_case(dims, M, n=n, nlist=nlist, nq=5)
    lists, codes = pqo.assign(oracle, 0, X, C_), pqo.encode(oracle, cb, X)
    mask = rv.byte_mask(np.random.default_rng(M), n, 0.5)
    h = _handle(X, C_, cb)
    h.set_filter(mask)
    for nprobe in nprobes:
        _check(oracle, h, cb, 0, Q, C_, lists, codes, mask, K, nprobe, ctx=f"M {M} nprobe {nprobe}")
    h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_filter_column_equals_set_filter_of_the_restated_predicate(oracle, parity):
    X, Q, C_, cb, lists, codes = parity
    n = X.shape[0]
    rng = np.random.default_rng(17)
    cols = {"int64": (rv.int64_edge_column(n), 2 ** 32), "float32": (rv.float32_edge_column(n), 0.25)}
    valid = rng.random(n) < 0.8
    byte_mask = fc.parity_masks()["50 % byte mask"]
    h, twin = _handle(X, C_, cb), _handle(X, C_, cb)

    def same_as_twin(mask, ctx):
        twin.set_filter(mask)
        assert h.nvisible() == twin.nvisible() == np.count_nonzero(mask), ctx
        assert_same(*h.search(Q, K, 3), *twin.search(Q, K, 3), ctx)
        assert h.last_search_stats() == twin.last_search_stats(), ctx

    for name, (col, val) in cols.items():
        for op in rv.OPS:
            for voff in (0, 3):
                h.filter_column(col, val, op, valid=rv.validity_bitmap(valid, voff), validity_offset=voff)
                same_as_twin(rv.predicate(col, val, op, valid), f"{name} op {op} validity offset {voff}")
        h.filter_column(col, val, rv.GE)  # no validity bitmap: every row is valid
        same_as_twin(rv.predicate(col, val, rv.GE), f"{name} GE, no validity")
    icol, ival = cols["int64"]
    fcol, fval = cols["float32"]
    # combine ANDs into a byte mask, and into the predicate before it.  The AND is simd.AndBytes', bitwise, and a match is the
    # byte 1: of the mask's bytes 1, 2, 0x80 and 0xFF only 1 and 0xFF keep a matching row visible
    h.set_filter(byte_mask)
    h.filter_column(icol, ival, rv.LT, valid=rv.validity_bitmap(valid, 3), validity_offset=3, combine=True)
    m1 = rv.and_bytes(byte_mask, rv.predicate(icol, ival, rv.LT, valid))
    assert 0 < m1.sum() < np.count_nonzero(byte_mask)
    same_as_twin(m1, "combine after a byte mask")
    h.filter_column(fcol, fval, "<=", combine=True)
    m2 = rv.and_bytes(m1, rv.predicate(fcol, fval, rv.LE))
    assert 0 < m2.sum() < m1.sum()
    same_as_twin(m2, "combine after a predicate")
    _check(oracle, h, cb, 0, Q, C_, lists, codes, m2, K, 3, ctx="combined, against the helper")
    # combine on a handle without a filter replaces
    h.set_filter(None)
    h.filter_column(fcol, fval, rv.GT, valid=rv.validity_bitmap(valid, 0), combine=True)
    same_as_twin(rv.predicate(fcol, fval, rv.GT, valid), "combine on no filter")
    with pytest.raises(TypeError):
        h.filter_column(icol.astype(np.int32), 5, rv.EQ)
    h.Close()
    twin.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ids", [False, True])
def test_adds_under_a_filter(oracle, parity, with_ids):
    """1000 rows, a 50 % mask, 2000 more rows with reserve never called: the 4096-row buffers do not change, so a third add takes
    the handle past them (3000 -> 5000 rows) under the active filter.  Every add moves every position of the list-major codes."""
    X, Q, C_, cb, lists, codes = parity
    rng = np.random.default_rng(7)
    more = rng.standard_normal((2000, X.shape[1])).astype(F)
    all_rows = np.concatenate([X, more])
    all_lists = np.concatenate([lists, pqo.assign(oracle, 0, more, C_)])
    all_codes = np.concatenate([codes, pqo.encode(oracle, cb, more)])
    ids = rng.permutation(1 << 20)[:all_rows.shape[0]].astype(np.int64) + (1 << 41) if with_ids else None
    sub = lambda a, b: None if ids is None else ids[a:b]
    mask = rv.byte_mask(rng, 1000, 0.5)
    h = _handle(X[:1000], C_, cb, ids=sub(0, 1000))
    h.set_filter(mask)
    before = h.hbm_bytes
    for n in (3000, 5000):
        h.add(all_rows[h.ntotal:n], sub(h.ntotal, n))
        full = np.concatenate([mask, np.ones(n - 1000, np.uint8)])
        assert h.ntotal == n and np.array_equal(h.assignments(), all_lists[:n]) and np.array_equal(h.codes(), all_codes[:n])
        assert np.array_equal(h.list_sizes(), np.bincount(all_lists[:n], minlength=C_.shape[0]))
        for nprobe in (3, 16):
            _check(oracle, h, cb, 0, Q, C_, all_lists[:n], all_codes[:n], full, K, nprobe, ids=sub(0, n), ctx=f"{n} rows nprobe {nprobe}")
    assert h.hbm_bytes > before
    h.reserve(20000)  # a change of capacity alone keeps the filter too
    _check(oracle, h, cb, 0, Q, C_, all_lists, all_codes, full, K, 3, ids=ids, ctx="after reserve")
    h.Close()


def test_a_filter_set_on_an_empty_handle_covers_what_is_added(oracle, parity):
    X, Q, C_, cb, lists, codes = parity
    h = _handle(X[:0], C_, cb)
    h.set_filter(np.zeros(0, np.uint8))
    assert h.nvisible() == 0
    lab, dist = h.search(Q, K, 3)
    assert (lab == -1).all() and (dist == pqo.FLT_MAX).all() and h.last_search_stats() == (Q.shape[0], 0, 0, 0)
    h.add(X[:300])
    assert h.nvisible() == 300
    _check(oracle, h, cb, 0, Q, C_, lists[:300], codes[:300], np.ones(300, np.uint8), K, 3, ctx="filter set on an empty handle")
    h.set_filter(np.zeros(300, np.uint8))  # nothing visible: all padding, no row scanned
    assert h.nvisible() == 0
    lab, dist = h.search(Q, K, 3)
    assert (lab == -1).all() and (dist == pqo.FLT_MAX).all() and h.last_search_stats()[:3] == (Q.shape[0], 0, 0)
    h.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_replace_and_clear(oracle, parity):
    X, Q, C_, cb, lists, codes = parity
    masks = fc.parity_masks()
    h, twin = _handle(X, C_, cb), _handle(X, C_, cb)
    assert h.nvisible() == X.shape[0]
    h.set_filter(masks["10 % byte mask"])
    _check(oracle, h, cb, 0, Q, C_, lists, codes, masks["10 % byte mask"], K, 3, ctx="first mask")
    h.set_filter(masks["50 % byte mask"])
    _check(oracle, h, cb, 0, Q, C_, lists, codes, masks["50 % byte mask"], K, 3, ctx="second mask")
    h.set_filter(None)
    assert h.nvisible() == h.ntotal == X.shape[0]
    for nprobe in (1, 3, 16):
        assert_same(*h.search(Q, K, nprobe), *twin.search(Q, K, nprobe), f"cleared, nprobe {nprobe}")
        assert h.last_search_stats() == twin.last_search_stats()
    h.Close()
    twin.Close()


def test_refusals_behind_a_live_handle(parity):
    from longbow_amd import _lib
    X, Q, C_, cb, lists, codes = parity
    n = X.shape[0]
    mask = fc.parity_masks()["50 % byte mask"]
    h = _handle(X, C_, cb)
    h.set_filter(mask)
    want = h.search(Q, K, 3)
    for bad in (mask[:-1], np.concatenate([mask, mask[:1]])):
        with pytest.raises(_lib.LongbowGPUError) as e:
            h.set_filter(bad)
        assert e.value.code == INVALID and "rows" in str(e.value)
        for col in (np.zeros(bad.size, np.int64), np.zeros(bad.size, F)):
            with pytest.raises(_lib.LongbowGPUError) as e:
                h.filter_column(col, 0, rv.EQ)
            assert e.value.code == INVALID and "rows" in str(e.value)
        assert h.nvisible() == np.count_nonzero(mask)
        assert_same(*h.search(Q, K, 3), *want, "after a refused length")
    col = np.zeros(n, np.int64)
    valid = np.full((n + 7) // 8, 0xFF, np.uint8)
    lib = h._lib
    assert lib.lb_gpu_ivfpq_filter_int64(h._h, col.ctypes.data, n, 0, 6, None, 0, 0) == INVALID
    assert lib.lb_gpu_ivfpq_filter_int64(h._h, col.ctypes.data, n, 0, -1, None, 0, 0) == INVALID
    assert lib.lb_gpu_ivfpq_filter_int64(h._h, col.ctypes.data, n, 0, 0, valid.ctypes.data, -1, 0) == INVALID
    assert lib.lb_gpu_ivfpq_filter_float32(h._h, col.ctypes.data, n, 0.0, 6, None, 0, 1) == INVALID
    assert h.nvisible() == np.count_nonzero(mask)
    assert_same(*h.search(Q, K, 3), *want, "after a refused op")
    h.Close()


def test_every_list_probed_without_the_coarse_search_under_a_mask(oracle):
    """2100 lists are more than the LB_MAX_K probes the coarse search returns: with all of them probed the probes are the lists"""
    X, Q, C_, cb = pqo.parity_case(8, 4, n=5000, nlist=2100, nq=5)
    lists, codes = pqo.assign(oracle, 0, X, C_), pqo.encode(oracle, cb, X)
    mask = rv.byte_mask(np.random.default_rng(21), 5000, 0.5)
    h = _handle(X, C_, cb)
    h.set_filter(mask)
    for nprobe in (2100, 5000, 40):
        _check(oracle, h, cb, 0, Q, C_, lists, codes, mask, K, nprobe, ctx=f"2100 lists, nprobe {nprobe}")
    h.Close()


def test_batches_and_concurrent_searches_under_a_mask(oracle, parity):
    X, Q, C_, cb, lists, codes = parity
    big = np.random.default_rng(8).standard_normal((1025, X.shape[1])).astype(F)
    mask = fc.parity_masks()["50 % byte mask"]
    h = _handle(X, C_, cb)
    h.set_filter(mask)
    ol, od, scanned = pfc.search_filtered(oracle, cb, 0, big, C_, lists, codes, mask, K, 3)
    for nq in (1, 1025):  # 1025 queries run as two batches
        lab, dist = h.search(big[:nq], K, 3)
        assert_same(lab, dist, ol[:nq], od[:nq], f"nq {nq}")
        assert h.last_search_stats()[:2] == (nq, int(scanned[:nq].sum()))
    out = [None] * 4

    def work(t):
        out[t] = h.search(big[t * 50:t * 50 + 200], K, 3)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for t in range(4):
        assert_same(*out[t], ol[t * 50:t * 50 + 200], od[t * 50:t * 50 + 200], f"thread {t}")
    h.Close()


def test_profiled_filter_call_and_search(oracle, parity):
    X, Q, C_, cb, lists, codes = parity
    mask = fc.parity_masks()["10 % byte mask"]
    h = _handle(X, C_, cb)
    h.set_filter(mask)
    want = h.search(Q, K, 3)
    stats = h.last_search_stats()
    assert h.last_build_timing() == 0.0  # nothing was profiled yet
    h.set_profiling(True)
    h.set_filter(mask)
    ms = h.last_build_timing()
    assert np.isfinite(ms) and ms >= 0
    _check(oracle, h, cb, 0, Q, C_, lists, codes, mask, K, 3, ctx="profiled")
    assert_same(*h.search(Q, K, 3), *want, "profiled against unprofiled")
    assert h.last_search_stats() == stats
    t = h.last_timing()
    assert len(t) == 5 and all(np.isfinite(x) and x >= 0 for x in t) and sum(t) > 0, t
    h.add(X[:10])  # an add under the filter builds the visible lists too
    assert h.nvisible() == np.count_nonzero(mask) + 10 and h.last_build_timing() >= 0
    h.Close()
