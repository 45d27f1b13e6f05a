"""Removal and compaction of the IVF-Flat handle (lb_gpu_ivf_remove*, _nlive, _ndeleted, _compact; lb_ivf_host.h, lb_remove.h) on
the GPU: every search answers the exact k-NN among the live, filter-visible rows of the probed lists, bit for bit, before and
after lb_gpu_ivf_compact.  The expected result is tests/ivf_remove_cases.py's search_live (the IVF oracle over the lists with the
removed rows taken out; tests/test_ivf_remove_semantics.py pins on the CPU that this is the search of the survivors alone, and the
shapes of the inputs below); labels and distances are compared for equality.  The shapes are the smallest at which each path can
go wrong: lists emptied by a removal, live lengths around the scan's 128-row tile and the selection's 16,384 LDS keys, an add that
grows the capacity over live bytes, compaction rounds of 7 rows whose sources overlap earlier destinations, rows of 24 bytes."""
import ctypes as C

import numpy as np
import pytest

from tests import ivf_oracle as io
from tests import ivf_remove_cases as vc
from tests import row_view_cases as rv
from tests.gpu_util import assert_same, diag_lib, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F, H, I8 = np.float32, np.float16, np.int8
INVALID = 1
FLT_MAX = io.FLT_MAX


def _handle(kind, rows, C_, metric=0, order=0, ids=None, lib=None):
    """kind: f32 / f16 / i8; rows of that element type"""
    from longbow_amd import ivf
    from longbow_amd.gpu import DataType
    lib = lib or gpu_or_skip()
    if kind == "i8":
        h = ivf.IVFFlatInt8(C_, metric, order, lib=lib)
    else:
        h = ivf.IVFFlat(C_, metric, order, lib=lib, dtype=DataType.Float16 if kind == "f16" else DataType.Float32)
    if rows.shape[0]:
        h.add(rows, ids)
    return h


def _typed(kind, X, Q, C_):
    """parity-like f32 inputs as the handle's rows, its queries, its centroids and what the oracle reads in place of the rows"""
    if kind == "f16":
        X16 = X.astype(H)
        return X16, Q, C_, X16.astype(F)
    return X, Q, C_, X


def _expect(oracle, kind, metric, order, Q, W, C_, lists, live, k, nprobe, ids=None, mask=None):
    fn = vc.search_live_i8 if kind == "i8" else vc.search_live
    return fn(oracle, metric, order, Q, W, C_, lists, live, k, nprobe, ids=ids, mask=mask)


def _stats_ok(h, Q, scanned, ctx):
    st = h.last_search_stats()
    assert st[:3] == (Q.shape[0], int(scanned.sum()), int(scanned.max())), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= vc.LDS_KEYS).sum()), (st, ctx)


def _check(oracle, h, kind, metric, order, Q, W, C_, lists, live, ks, nprobe, ids=None, mask=None, ctx=""):
    """the searches at every k of ks against one oracle call at the largest (a smaller k's answer is its prefix), nvisible and the
    counters: the rows scanned are the live and visible ones alone -> rows scanned per query"""
    ol, od, scanned = _expect(oracle, kind, metric, order, Q, W, C_, lists, live, max(ks), nprobe, ids=ids, mask=mask)
    assert h.nvisible() == np.count_nonzero(vc.visible(live, mask)), ctx
    for k in ks:
        lab, dist = h.search(Q, k, nprobe)
        assert_same(lab, dist, ol[:, :k], od[:, :k], f"{ctx} k {k}")
        _stats_ok(h, Q, scanned, f"{ctx} k {k}")
    return scanned


_counts = vc.counts


def _flat(kind, dim, metric, order, rows):
    from longbow_amd import gpu
    if kind == "i8":
        idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=dim, Metric=metric, DataType=gpu.DataType.Int8))
    else:
        idx = new_index(dim, metric, order)
    idx.Add(None, rows)
    return idx


# ---- a. read-back ---------------------------------------------------------------------------------------------------------
def _readback(oracle, kind, metric, name):
    rows, Q0, C_, W, lists = vc.parity(oracle, kind, metric)
    n, nlist = rows.shape[0], C_.shape[0]
    removed = vc.readback_sets(lists)[name]
    live = vc.live_mask(n, removed)
    Q = Q0.copy()
    if removed.size:
        Q[0] = rows[removed[len(removed) // 2]].astype(Q.dtype)  # query 0 is a removed row's own vector
    h = _handle(kind, rows, C_, metric)
    flat = _flat(kind, rows.shape[1], metric, 0, rows) if kind != "f16" else None
    try:
        assert np.array_equal(h.assignments(), lists)  # (as int8 and float16 rows too: the case keeps its lists)
        assert _counts(h) == (n, n, 0)
        thrice = np.concatenate([removed, removed[::-1], removed])  # each row three times: removed once
        assert h.remove_rows(thrice) == removed.size
        assert h.remove_rows(removed) == 0 and h.remove(removed) == 0  # (no ids: labels are positions)
        assert _counts(h) == (n, n - removed.size, removed.size) and h.nvisible() == n - removed.size
        # positions do not move: what addresses the lists keeps counting the removed rows
        assert np.array_equal(h.assignments(), lists) and np.array_equal(h.list_sizes(), np.bincount(lists, minlength=nlist))
        if flat is not None:
            assert flat.remove_rows(removed) == removed.size
        for nprobe in vc.NPROBES:
            _check(oracle, h, kind, metric, 0, Q, W, C_, lists, live, vc.KS, nprobe, ctx=f"{kind} {name} metric {metric} nprobe {nprobe}")
            if nprobe == nlist and flat is not None:
                for k in vc.KS:
                    assert_same(*h.search(Q, k, nprobe), *flat.SearchBatch(Q, k), f"{name}: the flat index, k {k}")
        # k = 2048 with every list probed returns every live row when there are no more than that
        lab, dist = h.search(Q[:2], 2048, nlist)
        ol, od, _ = _expect(oracle, kind, metric, 0, Q[:2], W, C_, lists, live, 2048, nlist)
        assert_same(lab, dist, ol, od, f"{name} k 2048")
        if live.sum() <= 2048:
            assert np.array_equal(np.sort(lab[0][lab[0] >= 0]), np.flatnonzero(live)), name
        if flat is not None:
            assert_same(lab, dist, *flat.SearchBatch(Q[:2], 2048), f"{name}: the flat index, k 2048")
        if name == "all":
            assert np.all(lab == -1) and np.all(dist == FLT_MAX)
        if removed.size:
            assert h.search(Q[:1], 1, nlist)[0][0, 0] != removed[len(removed) // 2]
    finally:
        h.Close()
        if flat is not None:
            flat.Close()


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("name", vc.READBACK_NAMES)
def test_readback(oracle, name, metric):
    _readback(oracle, "f32", metric, name)


@pytest.mark.parametrize("kind,metric", [("f16", 1), ("i8", 0), ("i8", 2)])
@pytest.mark.parametrize("name", vc.READBACK_NAMES)
def test_typed_rows(oracle, name, kind, metric):
    _readback(oracle, kind, metric, name)


# ---- b. live lengths at the edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("choice", ["first rows", "random rows"])
@pytest.mark.parametrize("kind", ["f32", "f16", "i8"])
def test_list_edges(oracle, kind, choice):
    X, Q, C_, owner = vc.edge_case_i8() if kind == "i8" else io.edge_case(vc.EDGE_COUNTS)
    rows, Q, C_, W = (X, Q, C_, X) if kind == "i8" else _typed(kind, X, Q, C_)
    removed = vc.edge_removed(owner, None if choice == "first rows" else np.random.default_rng(6))
    live = vc.live_mask(owner.size, removed)
    h = _handle(kind, rows, C_)
    try:
        assert h.remove_rows(removed) == removed.size
        assert h.list_sizes().tolist() == list(vc.EDGE_COUNTS)
        for nprobe in (len(vc.EDGE_COUNTS), 2):
            _check(oracle, h, kind, 0, 0, Q, W, C_, owner, live, (10, 200), nprobe, ctx=f"{kind} {choice} nprobe {nprobe}")
        scanned = _check(oracle, h, kind, 0, 0, Q, W, C_, owner, live, (10,), 1, ctx=f"{kind} {choice} nprobe 1")
        assert scanned.tolist() == list(vc.EDGE_KEEP)
        lab, dist = h.search(Q, 10, 1)
        assert (lab[0] == -1).all() and (dist[0] == FLT_MAX).all()  # a probed list with no live row: all padding
        assert lab[1, 0] == np.flatnonzero((owner == 1) & (live != 0))[0] and (lab[1, 1:] == -1).all()
    finally:
        h.Close()


def test_selection_boundary(oracle):
    """50,000 rows.  List 0 is taken down to 16,385, 16,384 and 16,383 live rows on one handle: the selection of the queries that
    probe it runs from global memory, then from LDS"""
    X, Q5, C_ = io.skew_case()
    Q = vc.skew_queries(Q5)
    lists = io.assign(oracle, 0, 0, X, C_)
    live = np.ones(X.shape[0], np.uint8)
    h = _handle("f32", X, C_)
    try:
        for keep0, rows in vc.skew_steps(lists):
            assert h.remove_rows(rows) == rows.size
            live[rows] = 0
            for q in (Q[:1], Q):
                scanned = _check(oracle, h, "f32", 0, 0, q, X, C_, lists, live, (1, 100, 2048), 1, ctx=f"{keep0} live in list 0, {q.shape[0]} queries")
                assert scanned.max() == keep0
            assert h.last_search_stats()[3] == (8 if keep0 <= vc.LDS_KEYS else 2)
    finally:
        h.Close()


# ---- c. filters -------------------------------------------------------------------------------------------------------------
def test_filters_never_resurrect(oracle):
    X, Q0, C_ = io.parity_case()
    n = X.shape[0]
    lists = vc.parity_lists(oracle, 0)
    removed = vc.removed_rows(n, "18pct")
    Q = vc.queries(X, Q0, removed)
    live = vc.live_mask(n, removed)
    m = vc.filter_mask(n).copy()
    m[removed[:50]] = 0x80  # filter bytes other than 1, on rows that go and on rows that stay
    m[np.flatnonzero(live)[:50]] = 0x80
    col = rv.int64_edge_column(n)
    valid = np.random.default_rng(17).random(n) < 0.8
    pred, pred_valid = rv.predicate(col, 5, rv.GE), rv.predicate(col, 5, rv.GE, valid)
    assert (pred[removed] != 0).any() and 0 < pred_valid.sum() < pred.sum() < n
    h = _handle("f32", X, C_)

    def check(mask, ctx):
        for nprobe in (4, 16):
            _check(oracle, h, "f32", 0, 0, Q, X, C_, lists, live, (10,), nprobe, mask=mask, ctx=f"{ctx} nprobe {nprobe}")

    try:
        h.set_filter(m)
        assert h.remove_rows(removed) == removed.size
        check(m, "filter then remove")
        h.set_filter(None)
        check(None, "filter cleared: exactly the live rows")
        h.set_filter(np.ones(n, np.uint8))
        check(None, "an all-ones filter")
        h.filter_column(col, 5, rv.GE)
        check(pred, "filter_column replace")
        h.set_filter(m)
        h.filter_column(col, 5, rv.GE, combine=True)
        check(rv.and_bytes(m, pred), "filter_column combine")  # (bytewise, as simd.AndBytes: 0x80 AND 1 is 0)
        h.set_filter(None)
        h.filter_column(col, 5, rv.GE, combine=True)  # AND into "the live rows"
        check(pred, "filter_column combine without a filter")
        h.filter_column(col, 5, rv.GE, valid=rv.validity_bitmap(valid, 3), validity_offset=3)
        check(pred_valid, "a validity bitmap")
        # a wrong-length mask is still refused, and changes nothing; filters keep taking ntotal values
        assert h._lib.lb_gpu_ivf_set_filter(h._h, m.ctypes.data, n - removed.size) == INVALID
        check(pred_valid, "after the refused mask")
        h.set_filter(None)
        assert h.nvisible() == n - removed.size and _counts(h) == (n, n - removed.size, removed.size)
        # a removal under a filter that hides the row already still removes it
        gone = np.flatnonzero(live)[:3]
        hide = np.ones(n, np.uint8)
        hide[gone] = 0
        h.set_filter(hide)
        assert h.remove_rows(gone) == 3
        h.set_filter(None)
        live[gone] = 0
        check(None, "removed while hidden")
    finally:
        h.Close()


# ---- d. adds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_filter", [False, True])
def test_adds_after_removal(oracle, with_filter):
    """1000 rows of which 18 % go, then 2000 more (the 4096-row buffers stay), then 2000 more (the capacity grows over the live
    bytes); with a filter on the first 1000 rows or without"""
    X, Q, C_ = io.parity_case()
    rng = np.random.default_rng(7)
    more = rng.standard_normal((2000, X.shape[1])).astype(F)
    all_rows = np.concatenate([X, more])
    all_lists = np.concatenate([vc.parity_lists(oracle, 0), io.assign(oracle, 0, 0, more, C_)])
    removed = vc.removed_rows(1000, "18pct")
    live = vc.live_mask(1000, removed)
    mask = rv.byte_mask(rng, 1000, 0.5) if with_filter else None
    h = _handle("f32", X[:1000], C_)
    try:
        if with_filter:
            h.set_filter(mask)
        assert h.remove_rows(removed) == removed.size
        before = h.hbm_bytes
        for n in (3000, 5000):
            h.add(all_rows[h.ntotal:n])
            live = np.concatenate([live, np.ones(n - live.size, np.uint8)])
            full = None if mask is None else np.concatenate([mask, np.ones(n - 1000, np.uint8)])
            assert _counts(h) == (n, n - removed.size, removed.size)
            assert np.array_equal(h.assignments(), all_lists[:n])
            assert np.array_equal(h.list_sizes(), np.bincount(all_lists[:n], minlength=C_.shape[0]))
            for nprobe in (4, 16):
                _check(oracle, h, "f32", 0, 0, Q, all_rows[:n], C_, all_lists[:n], live, (10,), nprobe, mask=full, ctx=f"{n} rows nprobe {nprobe}")
        assert h.hbm_bytes > before
        # the new rows are live: they can be removed, and a removed old row stays gone
        assert h.remove_rows([removed[0], 1000, 4999]) == 2
        live[[1000, 4999]] = 0
        h.reserve(20000)  # a change of capacity alone keeps the live bytes too
        _check(oracle, h, "f32", 0, 0, Q, all_rows, C_, all_lists, live, (10,), 4, mask=full, ctx="after reserve")
    finally:
        h.Close()


# ---- e. ids -----------------------------------------------------------------------------------------------------------------
def test_ids(oracle):
    import torch
    X, Q0, C_ = io.parity_case()
    n = X.shape[0]
    lists = vc.parity_lists(oracle, 0)
    ids = vc.ids_for(n).copy()
    ids[777] = ids[2345]  # one id carried by two rows
    removed = vc.removed_rows(n, "18pct")
    removed = removed[(removed != 777) & (removed != 2345)]
    Q = vc.queries(X, Q0, removed)
    live = vc.live_mask(n, removed)
    a, b, c = _handle("f32", X, C_, ids=ids), _handle("f32", X, C_, ids=ids), _handle("f32", X, C_)

    def check(h, vis, labels, ctx):
        _check(oracle, h, "f32", 0, 0, Q, X, C_, lists, vis, (10,), 4, ids=labels, ctx=ctx)

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
        assert c.remove(np.concatenate([removed, [-1, n]])) == removed.size
        check(c, live, None, "remove on a handle without ids")
        d_more = torch.from_numpy(more).cuda()
        torch.cuda.synchronize()
        assert c.remove_device(d_more.numel(), d_more.data_ptr()) == more.size
        check(c, live_b, None, "remove_device on a handle without ids")
        # null pointers behind a live handle: refused, nothing written, nothing removed
        got = C.c_int64(-77)
        for name in ("lb_gpu_ivf_remove", "lb_gpu_ivf_remove_device", "lb_gpu_ivf_remove_rows"):
            assert getattr(c._lib, name)(c._h, 3, None, C.byref(got)) == INVALID and got.value == -77
            assert getattr(c._lib, name)(c._h, -1, more.ctypes.data, C.byref(got)) == INVALID and got.value == -77
            assert getattr(c._lib, name)(c._h, 0, None, C.byref(got)) == 0 and got.value == 0
            got.value = -77
        assert c.ndeleted() == removed.size + more.size
    finally:
        for h in (a, b, c):
            h.Close()


# ---- f. compaction ----------------------------------------------------------------------------------------------------------
def _search_device(h, Q, k, nprobe):
    import torch
    dQ = torch.from_numpy(np.array(Q, F)).cuda()  # (a copy: the shared inputs are read-only)
    dD = torch.full((Q.shape[0], k), -5.0, dtype=torch.float32, device="cuda")
    dL = torch.full((Q.shape[0], k), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h.search_device(Q.shape[0], dQ.data_ptr(), k, nprobe, dD.data_ptr(), dL.data_ptr())
    return dL.cpu().numpy(), dD.cpu().numpy()


@pytest.mark.parametrize("with_filter", [False, True])
@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("name", list(vc.FRACTIONS))
def test_compact(oracle, name, with_ids, with_filter):
    X, Q0, C_ = io.parity_case()
    n = X.shape[0]
    lists = vc.parity_lists(oracle, 0)
    removed = vc.removed_rows(n, name)
    Q = vc.queries(X, Q0, removed)
    live = vc.live_mask(n, removed)
    keep = np.flatnonzero(live)
    ids = vc.ids_for(n) if with_ids else None
    ls = None if ids is None else ids[keep]
    m = vc.filter_mask(n) if with_filter else None
    ms = None if m is None else m[keep]
    h, fresh = _handle("f32", X, C_, ids=ids), _handle("f32", X[keep], C_, ids=ls)
    try:
        if with_filter:
            h.set_filter(m)
            fresh.set_filter(ms)
        assert h.remove_rows(removed) == removed.size
        old = h.compact()
        assert np.array_equal(old, keep)
        assert _counts(h) == (keep.size, keep.size, 0)
        assert np.array_equal(h.assignments(), lists[keep]) and np.array_equal(h.list_sizes(), np.bincount(lists[keep], minlength=C_.shape[0]))
        vc.same_handles(h, fresh, Q, f"{name} compacted")
        _check(oracle, h, "f32", 0, 0, Q, X[keep], C_, lists[keep], np.ones(keep.size, np.uint8), (10,), 4, ids=ls, mask=ms, ctx=f"{name}: the oracle over the survivors")
        assert_same(*_search_device(h, Q, 10, 4), *fresh.search(Q, 10, 4), f"{name}: the device-pointer search")
        assert np.array_equal(h.compact(), np.arange(keep.size)) and _counts(h) == (keep.size, keep.size, 0)  # a second one: a no-op
        vc.same_handles(h, fresh, Q, f"{name} compacted twice", ks=(10,), nprobes=(4,))
        if with_filter:  # the filter that came along can be cleared and replaced
            h.set_filter(None)
            fresh.set_filter(None)
            vc.same_handles(h, fresh, Q, f"{name} filter cleared", ks=(10,), nprobes=(4,))
        # adds work afterwards, and removals again
        extra = np.random.default_rng(11).standard_normal((700, X.shape[1])).astype(F)
        eids = None if ids is None else np.arange(700, dtype=np.int64) + 7 * 10 ** 12
        for x in (h, fresh):
            x.add(extra, eids)
            assert x.remove_rows([0, keep.size + 5]) == 2
        vc.same_handles(h, fresh, Q, f"{name}: add and remove after compaction", ks=(10,), nprobes=(4, 16))
        X3 = np.concatenate([X[keep], extra])
        l3 = np.concatenate([lists[keep], io.assign(oracle, 0, 0, extra, C_)])
        live3 = vc.live_mask(X3.shape[0], [0, keep.size + 5])
        _check(oracle, h, "f32", 0, 0, Q, X3, C_, l3, live3, (10,), 4, ids=None if ids is None else np.concatenate([ls, eids]), ctx=f"{name}: after the add")
    finally:
        h.Close()
        fresh.Close()


def test_compact_edges(oracle):
    X, Q, C_ = io.parity_case()
    n = X.shape[0]
    lists = vc.parity_lists(oracle, 0)
    h = _handle("f32", X, C_)
    try:
        before = h.search(Q, 10, 4)
        assert np.array_equal(h.compact(), np.arange(n))  # nothing removed: a no-op
        assert _counts(h) == (n, n, 0)
        assert_same(*h.search(Q, 10, 4), *before, "no-op compaction")
        # cap < nlive: refused with a text, the handle unchanged
        assert h.remove_rows([5, 6, 7]) == 3
        old = np.full(n, -7, np.int64)
        assert h._lib.lb_gpu_ivf_compact(h._h, old.ctypes.data, n - 4) == INVALID
        assert b"old_rows" in h._lib.lb_gpu_ivf_last_error(h._h)
        assert np.all(old == -7) and _counts(h) == (n, n - 3, 3)
        live = vc.live_mask(n, [5, 6, 7])
        _check(oracle, h, "f32", 0, 0, Q, X, C_, lists, live, (10,), 4, ctx="after the refused compaction")
        # old_rows may be null
        assert h._lib.lb_gpu_ivf_compact(h._h, None, 0) == 0
        assert _counts(h) == (n - 3, n - 3, 0)
        keep = np.flatnonzero(live)
        _check(oracle, h, "f32", 0, 0, Q, X[keep], C_, lists[keep], np.ones(keep.size, np.uint8), (10,), 4, ctx="old_rows null")
        # everything removed: empty, and it takes adds again
        assert h.remove(np.arange(n - 3)) == n - 3
        lab, dist = h.search(Q[:2], 5, 4)
        assert np.all(lab == -1) and np.all(dist == FLT_MAX) and h.nvisible() == 0
        assert h.compact().size == 0 and _counts(h) == (0, 0, 0) and h.list_sizes().sum() == 0
        lab, dist = h.search(Q[:2], 5, 4)
        assert np.all(lab == -1) and np.all(dist == FLT_MAX)
        h.add(X[:100])
        assert _counts(h) == (100, 100, 0) and h.nvisible() == 100
        _check(oracle, h, "f32", 0, 0, Q, X[:100], C_, lists[:100], np.ones(100, np.uint8), (10,), 4, ctx="add into the emptied handle")
        assert h.remove_rows([99]) == 1 and h.compact().tolist() == list(range(99))
    finally:
        h.Close()


@pytest.mark.parametrize("round_rows", [7, 64])
@pytest.mark.parametrize("name", list(vc.overlap_sets(8)))
@pytest.mark.parametrize("kind", ["f32", "i8"])
def test_compact_rounds(oracle, kind, name, round_rows):
    """many rounds, a partial last one, sources that overlap the destinations of earlier rounds; int8 rows of 24 bytes, which the
    gather moves in 8-byte pieces and the scan reads in its one-lane form"""
    lib = diag_lib()
    if kind == "i8":
        X, Q, C_ = io.parity_case(1000, 24, 7, 9, seed=24)
        rows, Q, C_ = vc.o8.to_i8(X, vc.I8_SCALE), vc.o8.to_i8(Q, vc.I8_SCALE), (C_ * F(vc.I8_SCALE)).astype(F)
    else:
        rows, Q, C_ = io.parity_case()
    n = rows.shape[0]
    ids = vc.ids_for(n)
    removed = vc.overlap_sets(n)[name]
    keep = np.flatnonzero(vc.live_mask(n, removed))
    m = vc.filter_mask(n)
    h, fresh = _handle(kind, rows, C_, ids=ids, lib=lib), _handle(kind, rows[keep], C_, ids=ids[keep], lib=lib)
    try:
        h.set_filter(m)  # rows, ids and mask bytes all move
        assert h.remove_rows(removed) == removed.size
        lib.lb_debug_set_compact_round_rows(round_rows)
        try:
            old = h.compact()
        finally:
            lib.lb_debug_set_compact_round_rows(0)
        assert np.array_equal(old, keep) and _counts(h) == (keep.size, keep.size, 0)
        fresh.set_filter(m[keep])
        vc.same_handles(h, fresh, Q, f"{kind} {name} rounds of {round_rows}, filtered", ks=(10,), nprobes=(2, C_.shape[0]))
        h.set_filter(None)
        fresh.set_filter(None)
        vc.same_handles(h, fresh, Q, f"{kind} {name} rounds of {round_rows}", ks=(10, 2048), nprobes=(C_.shape[0],))  # every row arrived
    finally:
        h.Close()
        fresh.Close()


# ---- g. the Python mirror ---------------------------------------------------------------------------------------------------
def test_python_mirror(oracle):
    from longbow_amd import ivf
    gpu_or_skip()
    X, Q, C_ = io.parity_case()
    n = X.shape[0]
    lists = vc.parity_lists(oracle, 0)
    ids = vc.ids_for(n)
    removed = vc.removed_rows(n, "18pct")
    live = vc.live_mask(n, removed)
    idx = ivf.IVFFlatIndex(X.shape[1], ivf.IVFFlatConfig(NClusters=16, NProbe=4), centroids=C_)
    try:
        idx.AddBatch(ids, X)
        with pytest.raises(RuntimeError):
            idx.Remove(ids[:1])
        idx.Build()
        assert idx.Remove(ids[removed]) == removed.size
        assert (idx.Size(), idx.nlive(), idx.ndeleted()) == (n, n - removed.size, removed.size)  # Size() keeps its meaning
        ol, od, _ = vc.search_live(oracle, 0, 0, Q, X, C_, lists, live, 10, 4, ids=ids)
        assert_same(*idx.SearchBatch(Q, 10), ol, od, "SearchBatch after Remove")
        assert np.array_equal(idx.Compact(), np.flatnonzero(live)) and idx.Size() == n - removed.size
        assert_same(*idx.SearchBatch(Q, 10), ol, od, "SearchBatch after Compact")
    finally:
        idx.Close()
