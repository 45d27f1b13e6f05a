"""Removal and compaction of the IVF-PQ handle plain ("pq") and residual ("rpq") and of the IVF-SQ8 handle ("sq8") on the GPU
(lb_gpu_ivfpq_* / lb_gpu_ivfsq8_* _remove*, _nlive, _ndeleted, _compact).  Every search answers the handle's exact k-NN among
the live, filter-visible rows of the probed lists, bit for bit, before and after compaction; the codes are kept and never computed again.  The expected result is each handle's oracle with
mask = live & filter (tests/ivf_code_remove_cases.py; tests/test_ivf_code_remove_semantics.py pins on the CPU that this is the
search of the survivors alone, and the shapes of the inputs below); labels and distances are compared for equality.  The shapes
are the smallest at which each path can go wrong: lists emptied by a removal, live lengths around each scan's tile and the
selection's 16,384 LDS keys, an add that grows the capacity over live bytes, compaction rounds of 7 rows whose sources overlap
earlier destinations, codes of 4, 16, 20 (stride 32) and 768 bytes."""
import ctypes as C

import numpy as np
import pytest

from tests import ivf_code_remove_cases as cc
from tests import row_view_cases as rv
from tests.gpu_util import assert_same, diag_lib, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = 1
FLT_MAX = cc.FLT_MAX
KINDS = list(cc.KINDS)


def _handle(c, rows=None, ids=None, lib=None):
    """a handle of the case's kind holding its rows (`rows`: those positions alone, in that order)"""
    h = c.k.handle(c.C, c.par, lib=lib or gpu_or_skip())
    X = c.X if rows is None else c.X[rows]
    if X.shape[0]:
        h.add(X, ids)
    return h


def _stats_ok(h, Q, scanned, ctx):
    st = h.last_search_stats()
    assert st[:3] == (Q.shape[0], int(scanned.sum()), int(scanned.max())), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= cc.LDS_KEYS).sum()), (st, ctx)


def _check(oracle, c, h, Q, live, ks, nprobe, ids=None, mask=None, rows=None, ctx=""):
    """the searches at every k of ks against one oracle call at the largest (a smaller k's answer is its prefix), nvisible and the
    counters: the rows scanned are the live and visible ones alone -> rows scanned per query.  rows: the positions of the case
    that the handle holds (None: all); live and mask are over those"""
    vis = cc.visible(live, mask)
    ol, od, scanned = c.search(oracle, Q, vis, max(ks), nprobe, ids=ids, rows=rows)
    assert h.nvisible() == np.count_nonzero(vis), ctx
    for k in ks:
        lab, dist = h.search(Q, k, nprobe)
        assert_same(lab, dist, ol[:, :k], od[:, :k], f"{ctx} k {k}")
        _stats_ok(h, Q, scanned, f"{ctx} k {k}")
    return scanned


def _search_device(h, Q, k, nprobe):
    import torch
    dQ = torch.from_numpy(np.array(Q, F)).cuda()  # (a copy: the shared inputs are read-only)
    dD = torch.full((Q.shape[0], k), -5.0, dtype=torch.float32, device="cuda")
    dL = torch.full((Q.shape[0], k), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h.search_device(Q.shape[0], dQ.data_ptr(), k, nprobe, dD.data_ptr(), dL.data_ptr())
    torch.cuda.synchronize()
    return dL.cpu().numpy(), dD.cpu().numpy()


def _unchanged(h, c, ctx, n=None):
    """what addresses the rows keeps counting the removed ones: assignments, list sizes and the codes themselves"""
    n = c.n if n is None else n
    assert np.array_equal(h.assignments(), c.lists[:n]), f"{ctx}: assignments"
    assert np.array_equal(h.list_sizes(), np.bincount(c.lists[:n], minlength=c.nlist)), f"{ctx}: list sizes"
    assert np.array_equal(h.codes(), c.codes[:n]), f"{ctx}: codes"


# ---- a. read-back ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.READBACK_NAMES)
@pytest.mark.parametrize("kind,shape", cc.SHAPES, ids=cc.SHAPE_IDS)
def test_readback(oracle, kind, shape, name):
    c = cc.parity(oracle, kind, shape)
    n, nlist = c.n, c.nlist
    removed = cc.readback_sets(c.lists)[name]
    live = cc.live_mask(n, removed)
    Q = cc.queries(c, removed)  # query 0 is a removed row's own vector
    h = _handle(c)
    flat = c.k.flat(c.codes, c.par, c.dims) if c.k.flat_equal else None
    try:
        _unchanged(h, c, "before")
        assert cc.counts(h) == (n, n, 0)
        thrice = np.concatenate([removed, removed[::-1], removed])  # each row three times: removed once
        assert h.remove_rows(thrice) == removed.size
        assert h.remove_rows(removed) == 0 and h.remove(removed) == 0  # (no ids: labels are positions)
        assert cc.counts(h) == (n, n - removed.size, removed.size) and h.nvisible() == n - removed.size
        _unchanged(h, c, name)
        if flat is not None:
            flat.set_filter(live)
        for nprobe in cc.NPROBES:
            _check(oracle, c, h, Q, live, cc.KS, nprobe, ctx=f"{kind} {shape} {name} nprobe {nprobe}")
            if nprobe == nlist and flat is not None:
                for k in cc.KS:
                    assert_same(*h.search(Q, k, nprobe), *flat.search(Q, k), f"{name}: the flat code handle under set_filter(live), k {k}")
        # k = 2048 with every list probed returns every live row when there are no more than that
        lab, dist = h.search(Q[:2], cc.K_ALL, nlist)
        ol, od, scanned = c.search(oracle, Q[:2], live, cc.K_ALL, nlist)
        assert_same(lab, dist, ol, od, f"{name} k 2048")
        _stats_ok(h, Q[:2], scanned, f"{name} k 2048")
        if live.sum() <= cc.K_ALL:
            assert np.array_equal(np.sort(lab[0][lab[0] >= 0]), np.flatnonzero(live)), name
        if flat is not None:
            assert_same(lab, dist, *flat.search(Q[:2], cc.K_ALL), f"{name}: the flat code handle, k 2048")
        if name == "all":
            assert np.all(lab == -1) and np.all(dist == FLT_MAX)
        if removed.size:
            assert not np.isin(h.search(Q[:1], 10, nlist)[0], removed).any()
        _unchanged(h, c, f"{name}, after the searches")
    finally:
        h.Close()
        if flat is not None:
            flat.Close()


# ---- b. live lengths at the edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("choice", ["first rows", "random rows"])
@pytest.mark.parametrize("keeps", ["A", "B"])
@pytest.mark.parametrize("kind", KINDS)
def test_list_edges(oracle, kind, keeps, choice):
    c = cc.edge(oracle, kind)
    keep = cc.edge_keeps(kind)[keeps]
    removed = cc.edge_removed(c.lists, keep, None if choice == "first rows" else np.random.default_rng(6))
    live = cc.live_mask(c.n, removed)
    reps = c.Q.shape[0] // c.nlist  # query i probes list i % nlist first
    h = _handle(c)
    try:
        assert h.remove_rows(removed) == removed.size
        _unchanged(h, c, f"{kind} {keeps} {choice}")
        _check(oracle, c, h, c.Q, live, (10, 200), c.nlist, ctx=f"{kind} {keeps} {choice} every list")
        _check(oracle, c, h, c.Q[:c.nlist], live, (10,), 2, ctx=f"{kind} {keeps} {choice} nprobe 2")
        scanned = _check(oracle, c, h, c.Q, live, (10, 200), 1, ctx=f"{kind} {keeps} {choice} nprobe 1")
        assert scanned.tolist() == list(keep) * reps
        lab, dist = h.search(c.Q, 10, 1)
        for l in np.flatnonzero(np.asarray(keep) == 0):  # a probed list with no live row, emptied or empty: all padding
            assert (lab[l] == -1).all() and (dist[l] == FLT_MAX).all()
        one = keep.index(1)
        assert lab[one, 0] == np.flatnonzero((c.lists == one) & (live != 0))[0] and (lab[one, 1:] == -1).all()
    finally:
        h.Close()


@pytest.mark.parametrize("kind", KINDS)
def test_selection_boundary(oracle, kind):
    """50,000 rows.  List 0 is taken down to 16,385, 16,384 and 16,383 live rows on one handle: the selection of the queries that
    probe it runs from global memory, then from LDS"""
    c = cc.skew(oracle, kind)
    live = np.ones(c.n, np.uint8)
    h = _handle(c)
    try:
        for keep0, rows in cc.skew_steps(c.lists):
            assert h.remove_rows(rows) == rows.size
            live[rows] = 0
            for q in (c.Q[:1], c.Q):
                scanned = _check(oracle, c, h, q, live, (1, 100, cc.K_ALL), 1, ctx=f"{kind}: {keep0} live in list 0, {q.shape[0]} queries")
                assert scanned.max() == keep0
            assert h.last_search_stats()[3] == (8 if keep0 <= cc.LDS_KEYS else 2)
    finally:
        h.Close()


# ---- c. filters -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_filters_never_resurrect(oracle, kind):
    c = cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])
    n = c.n
    removed = cc.removed_rows(n, "18pct")
    Q = cc.queries(c, removed)
    live = cc.live_mask(n, removed)
    m = cc.filter_mask(n).copy()
    m[removed[:50]] = 0x80  # filter bytes other than 1, on rows that go and on rows that stay
    m[np.flatnonzero(live)[:50]] = 0x80
    col = rv.int64_edge_column(n)
    valid = np.random.default_rng(17).random(n) < 0.8
    pred, pred_valid = rv.predicate(col, 5, rv.GE), rv.predicate(col, 5, rv.GE, valid)
    assert (pred[removed] != 0).any() and 0 < pred_valid.sum() < pred.sum() < n
    h, other = _handle(c), _handle(c)

    def check(x, mask, ctx):
        for nprobe in (4, 16):
            _check(oracle, c, x, Q, live, (10,), nprobe, mask=mask, ctx=f"{kind} {ctx} nprobe {nprobe}")

    try:
        h.set_filter(m)                                    # the filter first, then the removal
        assert h.remove_rows(removed) == removed.size
        check(h, m, "filter then remove")
        assert other.remove_rows(removed) == removed.size  # the removal first, then the filter
        other.set_filter(m)
        check(other, m, "remove then filter")
        h.set_filter(None)
        check(h, None, "filter cleared: exactly the live rows")
        h.set_filter(np.ones(n, np.uint8))
        check(h, None, "an all-ones filter")
        h.filter_column(col, 5, rv.GE)
        check(h, pred, "filter_column replace")
        h.set_filter(m)
        h.filter_column(col, 5, rv.GE, combine=True)
        check(h, rv.and_bytes(m, pred), "filter_column combine")  # (bytewise, as simd.AndBytes: 0x80 AND 1 is 0)
        h.set_filter(None)
        h.filter_column(col, 5, rv.GE, combine=True)  # AND into "the live rows"
        check(h, pred, "filter_column combine without a filter")
        h.filter_column(col, 5, rv.GE, valid=rv.validity_bitmap(valid, 3), validity_offset=3)
        check(h, pred_valid, "a validity bitmap")
        # a wrong-length mask is still refused, and changes nothing; filters keep taking ntotal values
        assert h._fn("set_filter")(h._h, m.ctypes.data, n - removed.size) == INVALID
        check(h, pred_valid, "after the refused mask")
        h.set_filter(None)
        assert h.nvisible() == n - removed.size and cc.counts(h) == (n, n - removed.size, removed.size)
        # a removal under a filter that hides the row already still removes it
        gone = np.flatnonzero(live)[:3]
        hide = np.ones(n, np.uint8)
        hide[gone] = 0
        h.set_filter(hide)
        assert h.remove_rows(gone) == 3
        h.set_filter(None)
        live[gone] = 0
        check(h, None, "removed while hidden")
        _unchanged(h, c, f"{kind} after the filters")
    finally:
        h.Close()
        other.Close()


# ---- d. adds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_adds_after_removal(oracle, kind, with_filter):
    """1000 rows of which 18 % go, then 2000 more (the 4096-row buffers stay), then 2000 more (the capacity grows over the live
    bytes); with a filter on the first 1000 rows or without.  Every add moves every position of a list-major copy"""
    c = cc.grown(oracle, kind)
    rng = np.random.default_rng(7)
    removed = cc.removed_rows(1000, "18pct")
    live = cc.live_mask(1000, removed)
    mask = rv.byte_mask(rng, 1000, 0.5) if with_filter else None
    first = np.arange(1000)
    h = _handle(c, rows=first)
    try:
        if with_filter:
            h.set_filter(mask)
        assert h.remove_rows(removed) == removed.size
        before = h.hbm_bytes
        full = None
        for n in (3000, 5000):
            h.add(c.X[h.ntotal:n])
            live = np.concatenate([live, np.ones(n - live.size, np.uint8)])
            full = None if mask is None else np.concatenate([mask, np.ones(n - 1000, np.uint8)])
            assert cc.counts(h) == (n, n - removed.size, removed.size)
            _unchanged(h, c, f"{kind} {n} rows", n=n)
            for nprobe in (4, 16):
                _check(oracle, c, h, c.Q, live, (10,), nprobe, mask=full, rows=np.arange(n), ctx=f"{kind} {n} rows nprobe {nprobe}")
        assert h.hbm_bytes > before
        # the new rows are live: they can be removed, and a removed old row stays gone
        assert h.remove_rows([removed[0], 1000, 4999]) == 2
        live[[1000, 4999]] = 0
        h.reserve(20000)  # a change of capacity alone keeps the live bytes too
        _check(oracle, c, h, c.Q, live, (10,), 4, mask=full, ctx=f"{kind} after reserve")
        _unchanged(h, c, f"{kind} after reserve")
    finally:
        h.Close()


# ---- e. ids -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_ids(oracle, kind):
    import torch
    c = cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])
    n = c.n
    ids = cc.ids_for(n).copy()  # negative values and values beyond 2^32
    ids[777] = ids[2345]  # one id carried by two rows
    removed = cc.removed_rows(n, "18pct")
    removed = removed[(removed != 777) & (removed != 2345)]
    Q = cc.queries(c, removed)
    live = cc.live_mask(n, removed)
    a, b, d = _handle(c, ids=ids), _handle(c, ids=ids), _handle(c)

    def check(h, vis, labels, ctx):
        _check(oracle, c, h, Q, vis, (10,), 4, ids=labels, ctx=f"{kind} {ctx}")

    try:
        want = np.concatenate([ids[removed], [-1, 123456789012345, ids[removed[0]]]])  # padding, an unknown id, a repeat
        assert a.remove(want) == removed.size
        check(a, live, ids, "remove by id")
        d_want = torch.from_numpy(want).cuda()
        torch.cuda.synchronize()
        assert b.remove_device(d_want.numel(), d_want.data_ptr()) == removed.size
        check(b, live, ids, "remove_device by id")
        assert a.remove([ids[777]]) == 2 and a.ndeleted() == removed.size + 2  # both rows under the id go
        live_a = live.copy()
        live_a[[777, 2345]] = 0
        check(a, live_a, ids, "an id on two rows")
        assert a.remove([ids[777], -1, 42]) == 0 and a.ndeleted() == removed.size + 2
        # positions on a handle with ids; more entries than one workgroup takes, out-of-range ones among them
        more = np.flatnonzero(live)[:300].astype(np.int64)
        assert b.remove_rows(np.concatenate([more, [-1, n, n + 5, -2 ** 40, 2 ** 40]])) == more.size
        live_b = live.copy()
        live_b[more] = 0
        check(b, live_b, ids, "remove_rows on a handle with ids")
        # without ids: remove == remove_rows, host and device forms
        assert d.remove(np.concatenate([removed, [-1, n]])) == removed.size
        check(d, live, None, "remove on a handle without ids")
        d_more = torch.from_numpy(more).cuda()
        torch.cuda.synchronize()
        assert d.remove_device(d_more.numel(), d_more.data_ptr()) == more.size
        check(d, live_b, None, "remove_device on a handle without ids")
        # null pointers behind a live handle: refused, nothing written, nothing removed
        got = C.c_int64(-77)
        for name in ("remove", "remove_device", "remove_rows"):
            assert d._fn(name)(d._h, 3, None, C.byref(got)) == INVALID and got.value == -77
            assert d._fn(name)(d._h, -1, more.ctypes.data, C.byref(got)) == INVALID and got.value == -77
            assert d._fn(name)(d._h, 0, None, C.byref(got)) == 0 and got.value == 0
            got.value = -77
        assert d.ndeleted() == removed.size + more.size
        for h in (a, b, d):
            _unchanged(h, c, f"{kind} ids")
    finally:
        for h in (a, b, d):
            h.Close()


# ---- f. compaction, in the diagnostic library with rounds of 7 rows --------------------------------------------------------
def _compact(lib, h):
    lib.lb_debug_set_compact_round_rows(cc.ROUND_ROWS)
    try:
        return h.compact()
    finally:
        lib.lb_debug_set_compact_round_rows(0)


@pytest.mark.parametrize("state", ["ids and a filter", "bare"])
@pytest.mark.parametrize("name", list(cc.overlap_sets(8)))
@pytest.mark.parametrize("kind", KINDS)
def test_compact_rounds(oracle, kind, name, state):
    """many rounds, a partial last one, sources that overlap the destinations of earlier rounds.  Afterwards the handle is what an
    add of the survivors' VECTORS makes: the same codes (for a residual handle: nothing needed encoding again), assignments, list
    sizes, visible rows and searches"""
    lib = diag_lib()
    c = cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])
    n = c.n
    dressed = state != "bare"
    ids = cc.ids_for(n) if dressed else None
    m = cc.filter_mask(n) if dressed else None
    removed = cc.overlap_sets(n)[name]
    keep = np.flatnonzero(cc.live_mask(n, removed))
    ls, ms = (None if ids is None else ids[keep]), (None if m is None else m[keep])
    Q = cc.queries(c, removed)
    h, fresh = _handle(c, ids=ids, lib=lib), _handle(c, rows=keep, ids=ls, lib=lib)
    try:
        if dressed:
            h.set_filter(m)  # codes, ids and mask bytes all move
            fresh.set_filter(ms)
        assert h.remove_rows(removed) == removed.size
        old = _compact(lib, h)
        assert np.array_equal(old, keep) and cc.counts(h) == (keep.size, keep.size, 0)
        assert np.array_equal(h.codes(), c.codes[keep]), "get_codes equals the old codes taken at old_rows"
        assert np.array_equal(h.assignments(), c.lists[keep]) and np.array_equal(h.list_sizes(), np.bincount(c.lists[keep], minlength=c.nlist))
        cc.same_handles(h, fresh, Q, f"{kind} {name} {state}, rounds of 7")
        _check(oracle, c, h, Q, np.ones(keep.size, np.uint8), (10,), 4, ids=ls, mask=ms, rows=keep, ctx=f"{kind} {name} {state}: the oracle over the survivors")
        assert_same(*_search_device(h, Q, 10, 4), *fresh.search(Q, 10, 4), f"{kind} {name}: the device-pointer search")
        assert np.array_equal(_compact(lib, h), np.arange(keep.size)) and cc.counts(h) == (keep.size, keep.size, 0)  # a second one: a no-op
        if dressed:  # the filter that came along can be cleared
            h.set_filter(None)
            fresh.set_filter(None)
        cc.same_handles(h, fresh, Q, f"{kind} {name} {state}, every row arrived", ks=(10, cc.K_ALL), nprobes=(c.nlist,))
        # adds work afterwards, and removals again
        extra = np.random.default_rng(11).standard_normal((700, c.dims)).astype(F)
        eids = None if ids is None else np.arange(700, dtype=np.int64) + 7 * 10 ** 12
        for x in (h, fresh):
            x.add(extra, eids)
            assert x.remove_rows([0, keep.size + 5]) == 2
        cc.same_handles(h, fresh, Q, f"{kind} {name} {state}: add and remove after compaction", ks=(10,), nprobes=(4, 16))
    finally:
        h.Close()
        fresh.Close()


@pytest.mark.parametrize("kind", KINDS)
def test_compact_edges(oracle, kind):
    lib = diag_lib()
    c = cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])
    n, Q = c.n, c.Q
    h = _handle(c, lib=lib)
    try:
        before = h.search(Q, 10, 4)
        assert np.array_equal(_compact(lib, h), np.arange(n))  # nothing removed: a no-op
        assert cc.counts(h) == (n, n, 0)
        assert_same(*h.search(Q, 10, 4), *before, "no-op compaction")
        # cap < nlive: refused with a text, the handle unchanged
        assert h.remove_rows([5, 6, 7]) == 3
        old = np.full(n, -7, np.int64)
        assert h._fn("compact")(h._h, old.ctypes.data, n - 4) == INVALID
        assert b"old_rows" in h._fn("last_error")(h._h)
        assert np.all(old == -7) and cc.counts(h) == (n, n - 3, 3)
        live = cc.live_mask(n, [5, 6, 7])
        _check(oracle, c, h, Q, live, (10,), 4, ctx=f"{kind} after the refused compaction")
        _unchanged(h, c, f"{kind} after the refused compaction")
        # old_rows may be null
        lib.lb_debug_set_compact_round_rows(cc.ROUND_ROWS)
        try:
            assert h._fn("compact")(h._h, None, 0) == 0
        finally:
            lib.lb_debug_set_compact_round_rows(0)
        assert cc.counts(h) == (n - 3, n - 3, 0)
        keep = np.flatnonzero(live)
        _check(oracle, c, h, Q, np.ones(keep.size, np.uint8), (10,), 4, rows=keep, ctx=f"{kind} old_rows null")
        assert np.array_equal(h.codes(), c.codes[keep])
        # everything removed: empty, and it takes adds again
        assert h.remove(np.arange(n - 3)) == n - 3
        lab, dist = h.search(Q[:2], 5, 4)
        assert np.all(lab == -1) and np.all(dist == FLT_MAX) and h.nvisible() == 0
        assert _compact(lib, h).size == 0 and cc.counts(h) == (0, 0, 0) and h.list_sizes().sum() == 0
        lab, dist = h.search(Q[:2], 5, 4)
        assert np.all(lab == -1) and np.all(dist == FLT_MAX)
        first = np.arange(100)
        h.add(c.X[:100])
        assert cc.counts(h) == (100, 100, 0) and h.nvisible() == 100
        _check(oracle, c, h, Q, np.ones(100, np.uint8), (10,), 4, rows=first, ctx=f"{kind} add into the emptied handle")
        assert np.array_equal(h.codes(), c.codes[:100])
        assert h.remove_rows([99]) == 1 and _compact(lib, h).tolist() == list(range(99))
    finally:
        h.Close()


# ---- g. search_refine -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_search_refine_across_a_compaction(oracle, kind):
    """the same rows leave the code handle and a gpu.Index; both are compacted (both stably): the two-stage result is the one of
    before, mapped through old_rows, and it holds live rows only"""
    c = cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])
    removed = cc.removed_rows(c.n, "18pct")
    Q = cc.queries(c, removed)
    h = _handle(c)
    index = new_index(c.dims)
    try:
        index.Add(None, c.X)
        assert h.remove_rows(removed) == removed.size and index.remove_rows(removed) == removed.size
        pre_l, pre_d = h.search_refine(index, Q, 10, 100, 4)
        assert (pre_l >= 0).all() and not np.isin(pre_l, removed).any()
        old = h.compact()
        assert np.array_equal(index.Compact(), old)
        post_l, post_d = h.search_refine(index, Q, 10, 100, 4)
        assert_same(cc.back(post_l, old), post_d, pre_l, pre_d, f"{kind}: search_refine after compacting both")
    finally:
        h.Close()
        index.Close()
