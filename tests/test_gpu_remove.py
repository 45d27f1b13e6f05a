"""Removal and compaction of the flat index (index_remove.hip, kernels_remove.hip; the filter calls of index.hip; the prepare
kernel of kernels_refine.hip) against the oracle: every search answers the exact k-NN among the live, filter-visible rows, bit
for bit, before and after lb_gpu_index_compact.  Inputs come from tests/remove_cases.py; tests/test_remove_semantics.py pins on
the CPU that the oracle over the survivors alone is the oracle over every row under the live mask."""
import ctypes as C

import numpy as np
import pytest

from tests import i8_oracle
from tests import remove_cases as rc
from tests.gpu_util import assert_same, diag_lib, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F, H, I8 = np.float32, np.float16, np.int8
L2, COS, DOT = rc.L2, rc.COS, rc.DOT
FLT_MAX = np.finfo(F).max
LB_ERR_INVALID_ARG = 1
_cache = {}


def expected(oracle, metric, Q, X, k, live, ids=None, order=0):
    return oracle.search_batch(metric, np.asarray(Q, F), np.asarray(X, F), k, order=order, mask=np.asarray(live, np.uint8), ids=ids,
                               nthreads=16)


def expected_cached(oracle, key, *args, **kw):
    """computed once, shared by the tests that need it, never written to"""
    if key not in _cache:
        oi, od = expected(oracle, *args, **kw)
        oi.setflags(write=False)
        od.setflags(write=False)
        _cache[key] = (oi, od)
    return _cache[key]


def check_grid(idx, oracle, metric, Q, X, live, ids, key, ctx, nqs=rc.NQS, ks=rc.KS):
    """every (nq, k): the top k of the first nq queries is a corner of the oracle's largest answer (canonical order)"""
    oi, od = expected_cached(oracle, key, metric, Q[:nqs[-1]], X, ks[-1], live, ids)
    for nq in nqs:
        for k in ks:
            lab, dist = idx.SearchBatch(Q[:nq], k)
            assert_same(lab, dist, oi[:nq, :k], od[:nq, :k], f"{ctx} nq {nq} k {k}")


def counts(idx):
    return idx.ntotal, idx.nlive(), idx.ndeleted()


# ---- a. read-back ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.readback_sets(rc.SMALL[0])))
def test_readback(oracle, name):
    gpu_or_skip()
    X, Q = rc.corpus(rc.SMALL)
    n = rc.SMALL[0]
    removed = rc.readback_sets(n)[name]
    live = rc.live_mask(n, removed)
    idx = new_index(rc.SMALL[1], L2)
    try:
        idx.Add(None, X)
        assert counts(idx) == (n, n, 0)
        thrice = np.concatenate([removed, removed[::-1], removed])  # each label three times: removed once
        assert idx.remove_rows(thrice) == removed.size
        assert counts(idx) == (n, n - removed.size, removed.size)
        assert idx.remove_rows(removed) == 0  # a second identical call
        assert idx.Remove(removed) == 0       # (no ids: labels are positions)
        assert counts(idx) == (n, n - removed.size, removed.size)
        lab, dist = idx.SearchBatch(Q[:1], 2048)
        got = np.sort(lab[0][lab[0] >= 0])
        want = np.flatnonzero(live)[:2048] if live.sum() <= 2048 else None
        if want is not None:
            assert np.array_equal(got, want), (name, np.setdiff1d(got, want)[:8], np.setdiff1d(want, got)[:8])
        if name == "all":
            assert np.all(lab == -1) and np.all(dist == FLT_MAX)
        oi, od = expected(oracle, L2, Q[:1], X, 2048, live)
        assert_same(lab, dist, oi, od, name)
    finally:
        idx.Close()


# ---- b. views -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, COS, DOT])
@pytest.mark.parametrize("name", list(rc.FRACTIONS))
def test_views(oracle, name, metric):
    gpu_or_skip()
    X, Q0 = rc.corpus(rc.MAIN)
    n = rc.MAIN[0]
    removed = rc.removed_rows(n, name)
    Q = rc.queries(X, Q0, removed)
    live = rc.live_mask(n, removed)
    idx = new_index(rc.MAIN[1], metric)
    try:
        idx.Add(None, X)
        assert idx.Remove(removed) == removed.size
        assert counts(idx) == (n, n - removed.size, removed.size)
        check_grid(idx, oracle, metric, Q, X, live, None, ("views", name, metric), f"{name} metric {metric}")
        lab, _ = idx.SearchBatch(Q[:1], 1)
        assert lab[0, 0] != removed[len(removed) // 2]  # query 0 is that row's own vector
    finally:
        idx.Close()


def test_views_odd_dimension(oracle):
    gpu_or_skip()
    X, Q0 = rc.corpus(rc.ODD)
    n = rc.ODD[0]
    removed = rc.removed_rows(n, "18pct")
    Q = rc.queries(X, Q0, removed)
    idx = new_index(rc.ODD[1], L2)
    try:
        idx.Add(None, X)
        assert idx.remove_rows(removed) == removed.size
        check_grid(idx, oracle, L2, Q, X, rc.live_mask(n, removed), None, ("odd",), "dim 100", nqs=(64,), ks=(10,))
    finally:
        idx.Close()


# ---- c. filters -----------------------------------------------------------------------------------------------------
def test_filters_never_resurrect(oracle):
    gpu_or_skip()
    X, Q0 = rc.corpus(rc.MAIN)
    n, d = rc.MAIN
    removed = rc.removed_rows(n, "18pct")
    Q = rc.queries(X, Q0, removed)[:8]
    live = rc.live_mask(n, removed)
    m = rc.filter_mask(n)
    m[removed[:50]] = 0x80  # filter bytes other than 1, on rows that go and on rows that stay
    m[np.flatnonzero(live)[:50]] = 0x80
    col = np.random.default_rng(9).integers(0, 100, n).astype(np.int64)
    pred = (col >= 40).astype(np.uint8)
    idx = new_index(d, L2)

    def check(vis, ctx, Xs=X):
        lab, dist = idx.SearchBatch(Q, 10)
        oi, od = expected(oracle, L2, Q, Xs, 10, vis)
        assert_same(lab, dist, oi, od, ctx)

    try:
        idx.Add(None, X)
        idx.set_filter(m)
        assert idx.Remove(removed) == removed.size
        check((m != 0) & (live != 0), "filter then remove")
        idx.set_filter(None)
        check(live, "filter cleared: removed rows stay gone")
        idx.set_filter(np.ones(n, np.uint8))
        check(live, "an all-ones filter")
        idx.filter_column(col, ">=", 40)
        check(pred & live, "filter_column replace")
        idx.set_filter(m)
        idx.filter_column(col, ">=", 40, combine=True)
        # (the chain ANDs bytewise, as simd.AndBytes does: a 0x80 filter byte AND a predicate's 1 is 0, removed or not)
        check((oracle.and_bytes(m, pred) != 0) & (live != 0), "filter_column combine")
        idx.set_filter(None)
        idx.filter_column(col, ">=", 40, combine=True)  # AND into "removed rows only"
        check(pred & live, "filter_column combine without a filter")
        # a wrong-length mask is still refused, and changes nothing
        assert idx._lib.lb_gpu_index_set_filter(idx._h, m.ctypes.data, n - removed.size) == LB_ERR_INVALID_ARG
        check(pred & live, "after the refused mask")
        # appended rows are live; a filter now has ntotal bytes
        rng = np.random.default_rng(10)
        X2 = np.concatenate([X, rng.random((500, d), dtype=F)])
        idx.set_filter(None)
        idx.Add(None, X2[n:])
        live2 = np.concatenate([live, np.ones(500, np.uint8)])
        assert counts(idx) == (n + 500, n + 500 - removed.size, removed.size)
        check(live2, "after Add", X2)
        assert idx._lib.lb_gpu_index_set_filter(idx._h, m.ctypes.data, n) == LB_ERR_INVALID_ARG
        m2 = rc.filter_mask(n + 500, seed=6)
        idx.set_filter(m2)
        check(m2 & live2, "a filter over the grown index", X2)
    finally:
        idx.Close()


# ---- d. ids ---------------------------------------------------------------------------------------------------------
def test_ids(oracle):
    gpu_or_skip()
    import torch
    X, Q0 = rc.corpus(rc.MAIN)
    n, d = rc.MAIN
    ids = rc.ids_for(n).copy()
    ids[777] = ids[12345]  # one id carried by two rows
    removed = rc.removed_rows(n, "18pct")
    removed = removed[(removed != 777) & (removed != 12345)]
    Q = rc.queries(X, Q0, removed)[:8]
    live = rc.live_mask(n, removed)
    a, b, c = new_index(d, L2), new_index(d, L2), new_index(d, L2)

    def check(idx, vis, labels, ctx):
        lab, dist = idx.SearchBatch(Q, 10)
        oi, od = expected(oracle, L2, Q, X, 10, vis, ids=labels)
        assert_same(lab, dist, oi, od, ctx)

    try:
        a.Add(ids, X)
        b.Add(ids, X)
        c.Add(None, X)
        want = np.concatenate([ids[removed], [-1, 123456789012345, ids[removed[0]]]])  # padding, an unknown id, a repeat
        assert a.Remove(want) == removed.size
        check(a, live, ids, "remove by id")
        d_want = torch.from_numpy(want).cuda()
        assert b.remove_device(d_want.numel(), d_want.data_ptr()) == removed.size
        check(b, live, ids, "remove_device by id")
        assert a.Remove([ids[777]]) == 2 and a.ndeleted() == removed.size + 2  # both rows under the id go
        live_a = live.copy()
        live_a[[777, 12345]] = 0
        check(a, live_a, ids, "an id on two rows")
        assert a.Remove([ids[777], -1, 42]) == 0
        # positions on an index with ids; more entries than one workgroup takes, out-of-range ones among them
        more = np.flatnonzero(live)[:300].astype(np.int64)
        assert b.remove_rows(np.concatenate([more, [-1, n, n + 5, -2 ** 40, 2 ** 40]])) == more.size
        live_b = live.copy()
        live_b[more] = 0
        check(b, live_b, ids, "remove_rows on an index with ids")
        # a set too large for the kernel's LDS copy
        big = np.flatnonzero(live_b)[::2][:5000]
        big = big[(big != 777) & (big != 12345)]  # (the id those two share would take both)
        assert b.Remove(ids[big]) == big.size
        live_b[big] = 0
        check(b, live_b, ids, "a set of 5000 ids")
        # without ids: remove == remove_rows, host and device forms
        assert c.Remove(np.concatenate([removed, [-1, n]])) == removed.size
        check(c, live, None, "remove on an index without ids")
        d_more = torch.from_numpy(more).cuda()
        assert c.remove_device(d_more.numel(), d_more.data_ptr()) == more.size
        lc = live.copy()
        lc[more] = 0
        check(c, lc, None, "remove_device on an index without ids")
    finally:
        a.Close()
        b.Close()
        c.Close()


# ---- e. compaction --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("name", list(rc.FRACTIONS))
def test_compact(oracle, name, with_ids):
    gpu_or_skip()
    X, Q0 = rc.corpus(rc.MAIN)
    n, d = rc.MAIN
    removed = rc.removed_rows(n, name)
    Q = rc.queries(X, Q0, removed)
    live = rc.live_mask(n, removed)
    keep = np.flatnonzero(live)
    ids = rc.ids_for(n) if with_ids else None
    m = rc.filter_mask(n)
    idx, fresh = new_index(d, L2), new_index(d, L2)
    try:
        idx.Add(ids, X)
        idx.set_filter(m)
        assert idx.remove_rows(removed) == removed.size
        old = idx.Compact()
        assert np.array_equal(old, keep)
        assert counts(idx) == (keep.size, keep.size, 0)
        Xs = X[keep]
        ls = None if ids is None else ids[keep]
        fresh.Add(ls, Xs)
        # the filter set before still hides the same survivors
        fresh.set_filter(m[keep])
        lab, dist = idx.SearchBatch(Q[:64], 10)
        oi, od = oracle.search_batch(L2, Q[:64], Xs, 10, mask=m[keep], ids=ls, nthreads=16)
        assert_same(lab, dist, oi, od, f"{name}: filter kept through compaction")
        fl, fd = fresh.SearchBatch(Q[:64], 10)
        assert_same(lab, dist, fl, fd, f"{name}: fresh index under the same filter")
        idx.set_filter(None)
        fresh.set_filter(None)
        oi, od = expected_cached(oracle, ("compact", name, with_ids), L2, Q, Xs, rc.KS[-1], np.ones(keep.size, np.uint8), ls)
        for nq in rc.NQS:
            for k in rc.KS:
                lab, dist = idx.SearchBatch(Q[:nq], k)
                assert_same(lab, dist, oi[:nq, :k], od[:nq, :k], f"{name} compacted nq {nq} k {k}")
                fl, fd = fresh.SearchBatch(Q[:nq], k)
                assert_same(lab, dist, fl, fd, f"{name} fresh nq {nq} k {k}")
        # Add after compaction, then a search
        extra = np.random.default_rng(11).random((700, d), dtype=F)
        eids = None if ids is None else np.arange(700, dtype=np.int64) + 7 * 10 ** 12
        idx.Add(eids, extra)
        X3 = np.concatenate([Xs, extra])
        l3 = None if ids is None else np.concatenate([ls, eids])
        assert counts(idx) == (keep.size + 700, keep.size + 700, 0)
        for nq in (1, 64):
            lab, dist = idx.SearchBatch(Q[:nq], 10)
            oi, od = oracle.search_batch(L2, Q[:nq], X3, 10, ids=l3, nthreads=16)
            assert_same(lab, dist, oi, od, f"{name}: Add after compaction nq {nq}")
    finally:
        idx.Close()
        fresh.Close()


def test_compact_edges(oracle):
    gpu_or_skip()
    X, Q = rc.corpus(rc.SMALL)
    n, d = rc.SMALL
    idx = new_index(d, L2)
    try:
        idx.Add(None, X)
        before = idx.SearchBatch(Q[:8], 10)
        assert np.array_equal(idx.Compact(), np.arange(n))  # nothing removed: a no-op
        assert counts(idx) == (n, n, 0)
        after = idx.SearchBatch(Q[:8], 10)
        assert_same(after[0], after[1], before[0], before[1], "no-op compaction")
        # cap < nlive: refused, the index unchanged
        assert idx.remove_rows([5, 6, 7]) == 3
        old = np.full(n, -7, np.int64)
        assert idx._lib.lb_gpu_index_compact(idx._h, old.ctypes.data, n - 4) == LB_ERR_INVALID_ARG
        assert np.all(old == -7) and counts(idx) == (n, n - 3, 3)
        live = rc.live_mask(n, [5, 6, 7])
        lab, dist = idx.SearchBatch(Q[:8], 10)
        oi, od = expected(oracle, L2, Q[:8], X, 10, live)
        assert_same(lab, dist, oi, od, "after the refused compaction")
        # old_rows may be null
        assert idx._lib.lb_gpu_index_compact(idx._h, None, 0) == 0
        assert counts(idx) == (n - 3, n - 3, 0)
        # everything removed: empty, and it takes Adds again
        assert idx.Remove(np.arange(n - 3)) == n - 3
        assert idx.Compact().size == 0 and counts(idx) == (0, 0, 0)
        lab, dist = idx.SearchBatch(Q[:2], 5)
        assert np.all(lab == -1) and np.all(dist == FLT_MAX)
        idx.Add(None, X[:100])
        lab, dist = idx.SearchBatch(Q[:8], 10)
        oi, od = oracle.search_batch(L2, Q[:8], X[:100], 10)
        assert_same(lab, dist, oi, od, "Add into the emptied index")
    finally:
        idx.Close()


def check_every_row_arrived(idx, oracle, q, Xs, ctx):
    dist = idx.Rerank(q, np.arange(Xs.shape[0], dtype=np.int64), want_score=False)
    assert np.array_equal(dist, oracle.batch_flat(L2, q, Xs, oracle.UNROLL4)), ctx


@pytest.mark.parametrize("shape", [rc.SMALL, rc.MAIN], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(rc.overlap_sets(rc.SMALL[0])))
def test_compact_overlap_rounds(oracle, name, shape):
    """rounds of 256 rows: many rounds, a partial last one, sources that overlap the destinations of earlier rounds"""
    lib = diag_lib()
    X, Q = rc.corpus(shape)
    n, d = shape
    removed = rc.overlap_sets(n)[name]
    keep = np.flatnonzero(rc.live_mask(n, removed))
    idx = new_index(d, L2, lib=lib)
    try:
        idx.Add(None, X)
        assert idx.remove_rows(removed) == removed.size
        lib.lb_debug_set_compact_round_rows(256)
        try:
            old = idx.Compact()
        finally:
            lib.lb_debug_set_compact_round_rows(0)
        assert np.array_equal(old, keep) and counts(idx) == (keep.size, keep.size, 0)
        check_every_row_arrived(idx, oracle, Q[0], X[keep], f"{name} {shape}")
        lab, dist = idx.SearchBatch(Q[:8], 10)
        oi, od = oracle.search_batch(L2, Q[:8], X[keep], 10, nthreads=16)
        assert_same(lab, dist, oi, od, f"{name} {shape}")
    finally:
        idx.Close()


def test_compact_hipmalloc_storage(oracle):
    """the corpus in one hipMalloc'd buffer (the mapping refused once): the same gather"""
    lib = diag_lib()
    X, Q = rc.corpus(rc.MAIN)
    n, d = rc.MAIN
    ids = rc.ids_for(n)
    removed = rc.overlap_sets(n)["every other"]
    keep = np.flatnonzero(rc.live_mask(n, removed))
    idx = new_index(d, L2, lib=lib)
    try:
        idx.Add(ids[:1000], X[:1000])
        try:
            lib.lb_debug_vmm_fail_next(1)
            idx.reserve(700_000)
        finally:
            lib.lb_debug_vmm_fail_next(0)
        idx.Add(ids[1000:], X[1000:])
        assert idx.remove_rows(removed) == removed.size
        lib.lb_debug_set_compact_round_rows(256)
        try:
            old = idx.Compact()
        finally:
            lib.lb_debug_set_compact_round_rows(0)
        assert np.array_equal(old, keep)
        check_every_row_arrived(idx, oracle, Q[0], X[keep], "hipMalloc storage")
        lab, dist = idx.SearchBatch(Q[:64], 10)
        oi, od = oracle.search_batch(L2, Q[:64], X[keep], 10, ids=ids[keep], nthreads=16)
        assert_same(lab, dist, oi, od, "hipMalloc storage")
    finally:
        idx.Close()


def test_compact_drops_the_nan_row(oracle):
    """a corpus whose only NaN row is removed and compacted away answers as the fresh index does, by the same routes"""
    gpu_or_skip()
    X0, Q = rc.corpus(rc.MAIN)
    n, d = rc.MAIN
    X = X0.copy()
    X[4321, 3] = np.nan
    keep = np.delete(np.arange(n), 4321)
    idx, fresh = new_index(d, L2), new_index(d, L2)
    try:
        idx.Add(None, X)
        fresh.Add(None, X[keep])
        assert idx.remove_rows([4321]) == 1
        lab, dist = idx.SearchBatch(Q[:64], 10)
        oi, od = expected(oracle, L2, Q[:64], X, 10, rc.live_mask(n, [4321]))
        assert_same(lab, dist, oi, od, "NaN row removed")
        idx.Compact()
        for nq in (1, 64):
            lab, dist = idx.SearchBatch(Q[:nq], 10)
            route = idx._lib.lb_gpu_index_last_route(idx._h)
            fl, fd = fresh.SearchBatch(Q[:nq], 10)
            assert_same(lab, dist, fl, fd, f"NaN row compacted away nq {nq}")
            assert route == fresh._lib.lb_gpu_index_last_route(fresh._h), nq
            oi, od = oracle.search_batch(L2, Q[:nq], X[keep], 10, nthreads=16)
            assert_same(lab, dist, oi, od, f"NaN row compacted away nq {nq}")
    finally:
        idx.Close()
        fresh.Close()


# ---- f. other element types -----------------------------------------------------------------------------------------
def typed_index(dim, metric, dtype):
    from longbow_amd import gpu
    return gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=dim, Metric=metric, DataType=dtype))


def test_f16_rows(oracle):
    gpu_or_skip()
    from longbow_amd import gpu
    X32, Q32 = rc.corpus(rc.MAIN)
    n, d = rc.MAIN
    X, Q = X32.astype(H), Q32.astype(H)
    removed = rc.removed_rows(n, "18pct")
    Q = Q.copy()
    Q[0] = X[removed[0]]
    live = rc.live_mask(n, removed)
    keep = np.flatnonzero(live)
    Xf, Qf = X.astype(F), Q.astype(F)
    idx = typed_index(d, L2, gpu.DataType.Float16)
    try:
        idx.Add(None, X)
        assert idx.Remove(removed) == removed.size
        for nq in (1, 64):
            lab, dist = idx.SearchBatch(Q[:nq], 10)
            oi, od = expected(oracle, L2, Qf[:nq], Xf, 10, live, order=oracle.UNROLL4)
            assert_same(lab, dist, oi, od, f"f16 removed nq {nq}")
        assert np.array_equal(idx.Compact(), keep)
        for nq in (1, 64):
            lab, dist = idx.SearchBatch(Q[:nq], 10)
            oi, od = oracle.search_batch(L2, Qf[:nq], Xf[keep], 10, order=oracle.UNROLL4, nthreads=16)
            assert_same(lab, dist, oi, od, f"f16 compacted nq {nq}")
    finally:
        idx.Close()


@pytest.mark.parametrize("shape", [rc.MAIN, (2049, 24)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_i8_rows(shape):
    """(2049 x 24: rows of 24 bytes, the gather's pieces narrower than 16 bytes)"""
    gpu_or_skip()
    from longbow_amd import gpu
    n, d = shape
    rng = np.random.default_rng(n + d)
    X = rng.integers(-128, 128, (n, d), dtype=np.int64).astype(I8)
    Q = rng.integers(-128, 128, (64, d), dtype=np.int64).astype(I8)
    removed = np.sort(rng.choice(n, int(round(n * 0.18)), replace=False)).astype(np.int64)
    Q[0] = X[removed[0]]
    keep = np.flatnonzero(rc.live_mask(n, removed))
    ids = rc.ids_for(n)
    idx = typed_index(d, L2, gpu.DataType.Int8)
    try:
        idx.Add(ids, X)
        assert idx.Remove(ids[removed]) == removed.size
        for nq in (1, 64):
            lab, dist = idx.SearchBatch(Q[:nq], 10)
            oi, od = i8_oracle.search(L2, Q[:nq], X, 10, ids=ids, visible=keep)
            assert_same(lab, dist, oi, od, f"i8 removed nq {nq}")
        assert np.array_equal(idx.Compact(), keep)
        for nq in (1, 64):
            lab, dist = idx.SearchBatch(Q[:nq], 10)
            oi, od = i8_oracle.search(L2, Q[:nq], X[keep], 10, ids=ids[keep])
            assert_same(lab, dist, oi, od, f"i8 compacted nq {nq}")
    finally:
        idx.Close()


# ---- g. refine ------------------------------------------------------------------------------------------------------
def test_refine_skips_removed_positions(oracle):
    gpu_or_skip()
    X, Q0 = rc.corpus(rc.MAIN)
    n, d = rc.MAIN
    removed = rc.removed_rows(n, "18pct")
    Q = Q0[:16]
    rng = np.random.default_rng(12)
    short = rng.integers(0, n, (16, 300)).astype(np.int64)
    short[:, :40] = removed[rng.integers(0, removed.size, (16, 40))]  # removed positions in every shortlist
    short[:, 7], short[:, 50] = -1, short[:, 51]
    scrubbed = np.where(np.isin(short, removed), -1, short)
    idx, ref = new_index(d, L2), new_index(d, L2)
    try:
        idx.Add(None, X)
        ref.Add(None, X)
        today = ref.Refine(Q, short, 20)
        got = idx.Refine(Q, short, 20)
        assert_same(got[0], got[1], today[0], today[1], "nothing removed: Refine as it was")
        assert idx.remove_rows(removed) == removed.size
        got = idx.Refine(Q, short, 20)
        want = ref.Refine(Q, scrubbed, 20)
        assert_same(got[0], got[1], want[0], want[1], "removed positions join the padding")
        same = idx.Refine(Q, scrubbed, 20)
        assert_same(got[0], got[1], same[0], same[1], "the same call with those entries replaced by -1")
        assert not np.isin(got[0], removed).any()
        for q in range(16):  # and both are the oracle's top 20 of the live entries
            S = np.unique(scrubbed[q][scrubbed[q] >= 0])
            oi, od, _ = oracle.topk_canonical(oracle.batch_flat(L2, Q[q], X[S], 0), 20)
            assert np.array_equal(got[0][q], S[oi]) and np.array_equal(got[1][q], od), q
        lists_all_removed = np.broadcast_to(removed[:300], (16, 300)).copy()
        lab, dist = idx.Refine(Q, lists_all_removed, 5)
        assert np.all(lab == -1) and np.all(dist == FLT_MAX)
    finally:
        idx.Close()
        ref.Close()
