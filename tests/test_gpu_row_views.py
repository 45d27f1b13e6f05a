"""Predicate masks and row views at their edges: kernels_filter.hip (match, and-bytes, the three compaction kernels) and
filter_column / lb_gpu_index_set_filter / rebuild_rowmap / finish_add in index.hip and row_view in lb_index.h, against the
oracle.  Inputs come from tests/row_view_cases.py; tests/test_row_view_semantics.py pins the oracle on the same inputs on the CPU.  Every
comparison is exact: mask bytes, label sets, and result lists bit for bit."""
import numpy as np
import pytest

from tests import row_view_cases as rc
from tests.gpu_util import assert_same, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
L2, COS, DOT = 0, 1, 2
FLT_MAX = np.finfo(F).max
CAND_F32_MFMA, CAND_SPLIT_INREG, CAND_AUTO, CAND_F16 = 0, 2, 3, 4  # lb_candidate_mode
LB_ERR_INVALID_ARG = 1


# ---- section 2: the match and and-bytes kernels ------------------------------------------------------------------------
def test_match_int64_edge_values(oracle):
    gpu_or_skip()
    from longbow_amd import simd
    col = rc.int64_edge_column()
    for val in rc.INT64_VALUES:
        for op in rc.OPS:
            dst = np.full(col.size, 7, np.uint8)
            simd.MatchInt64(col, val, op, dst)
            assert np.array_equal(dst, oracle.match_int64(col, val, op)), (val, op, np.flatnonzero(dst != oracle.match_int64(col, val, op))[:8])


def test_match_float32_edge_values(oracle):
    gpu_or_skip()
    from longbow_amd import simd
    col = rc.float32_edge_column()
    for val in rc.FLOAT32_VALUES:
        for op in rc.OPS:
            dst = np.full(col.size, 7, np.uint8)
            simd.MatchFloat32(col, val, op, dst)
            exp = oracle.match_float32(col, val, op)
            assert np.array_equal(dst, exp), (val, op, np.flatnonzero(dst != exp)[:8])


@pytest.mark.parametrize("kind", ["int64", "float32"])
def test_match_kernel_second_round(oracle, kind):
    """n beyond 4096 workgroups x 256 threads x 16 elements: the grid-stride loop's second iteration, three full groups and a
    partial one.  dst starts as 7, so an element that never comes back fails; an element no round wrote holds whatever the
    device buffer held, and EQ (constant part all 1) and LT (all 0) cannot both agree with that."""
    gpu_or_skip()
    from longbow_amd import simd
    if kind == "int64":
        col, val, match, ref = rc.big_int64_column(), rc.BIG_INT64_VALUE, simd.MatchInt64, oracle.match_int64
    else:
        col, val, match, ref = rc.big_float32_column(), rc.BIG_FLOAT32_VALUE, simd.MatchFloat32, oracle.match_float32
    assert col.size > rc.MATCH_ROUND
    for op in (rc.EQ, rc.LT):
        dst = np.full(col.size, 7, np.uint8)
        match(col, val, op, dst)
        exp = ref(col, val, op)
        assert np.array_equal(dst, exp), (op, np.flatnonzero(dst != exp)[:8])


@pytest.mark.parametrize("n", [1, 255, 256, 257, rc.AND_ROUND + 77])
def test_and_bytes_arbitrary_bytes(oracle, n):
    """bytes 0..255 (the reference ANDs bitwise); the last size runs and_bytes_kernel's loop a second time"""
    gpu_or_skip()
    from longbow_amd import simd
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n).astype(np.uint8)
    b = rng.integers(0, 256, n).astype(np.uint8)
    b0 = b.copy()
    exp = oracle.and_bytes(a, b)
    simd.AndBytes(a, b)
    assert np.array_equal(a, exp), np.flatnonzero(a != exp)[:8]
    assert np.array_equal(b, b0)


# ---- shared corpora (computed once, never written to) ---------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """2049 x 8: searched with k = 2048, the labels that are not -1 are exactly the visible rows"""
    rng = np.random.default_rng(100)
    X, q = rng.random((2049, 8), dtype=F), rng.random((1, 8), dtype=F)
    X.setflags(write=False)
    return X, q


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(101)
    n, d = 20000, 32
    X, Q = rng.random((n, d), dtype=F), rng.random((385, d), dtype=F)
    Q[0] = X[n // 3]  # the row rc.structured_masks' "all but one" hides is query 0's nearest neighbour
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


def check_mask_readback(idx, oracle, X, q, expected, ctx):
    """the view the index holds is `expected`: the set of labels of a k = 2048 search over at most 2049 rows, and the list"""
    expected = np.asarray(expected, np.uint8)
    lab, dist = idx.SearchBatch(q, 2048)
    vis = np.flatnonzero(expected)
    assert vis.size <= 2048
    got = np.sort(lab[0][lab[0] >= 0])
    assert np.array_equal(got, vis), f"{ctx}: shown but hidden {np.setdiff1d(got, vis)[:8]}, hidden but visible {np.setdiff1d(vis, got)[:8]}"
    oi, od = oracle.search_batch(L2, q, X[:expected.size], 2048, mask=expected)
    assert_same(lab, dist, oi, od, ctx)


def check_lists(idx, oracle, metric, Q, X, k, mask, ctx, order=0):
    mask = (np.asarray(mask) != 0).astype(np.uint8)
    lab, dist = idx.SearchBatch(Q, k)
    oi, od = oracle.search_batch(metric, np.asarray(Q, F), np.asarray(X, F), k, order=order, mask=mask, nthreads=16)
    assert_same(lab, dist, oi, od, ctx)
    nv = int(mask.sum())
    if nv < k:  # the padding behind a view shorter than k
        assert np.all(lab[:, nv:] == -1) and np.all(dist[:, nv:] == FLT_MAX), ctx
        assert np.all(lab[:, :nv] >= 0), ctx
    return lab, dist


# ---- section 3: validity bitmaps, offsets and AND chains through the index ------------------------------------------
OFFSETS = (0, 1, 7, 8, 13, 67)


@pytest.mark.parametrize("kind", ["int64", "float32"])
@pytest.mark.parametrize("n", [2000, 1999, 2001, 2047, 2049])
def test_validity_offsets_and_chains(oracle, small, n, kind):
    gpu_or_skip()
    X, q = small
    rng = np.random.default_rng(n * 2 + (kind == "int64"))
    if kind == "int64":
        cols = [rng.permutation(rc.int64_edge_column(n)) for _ in range(2)]
        values = rc.INT64_VALUES
    else:
        cols = [rng.permutation(rc.float32_edge_column(n)) for _ in range(2)]
        values = rc.FLOAT32_VALUES
    idx = new_index(8, L2)
    try:
        idx.Add(None, X[:n])
        for j, off in enumerate(OFFSETS):
            op, op2 = rc.OPS[j], rc.OPS[(j + 3) % 6]
            val, val2 = values[j % len(values)], values[(j + 4) % len(values)]
            valid, valid2 = rng.random(n) > 0.25, rng.random(n) > 0.25
            valid[[0, n - 1]] = [j % 2 == 0, j % 2 == 1]  # both ends of the bitmap both ways over the offsets
            bm, off2 = rc.validity_bitmap(valid, off), OFFSETS[(j + 1) % len(OFFSETS)]
            bm2 = rc.validity_bitmap(valid2, off2)
            ctx = f"{kind} n {n} offset {off} op {op} value {val!r}"
            first = rc.predicate(cols[0], val, op, valid)
            # combine = False: replaces whatever the earlier cases left
            idx.filter_column(cols[0], op, val, validity=bm, validity_offset=off)
            check_mask_readback(idx, oracle, X, q, first, ctx + " replace")
            # combine = True on top of a set_filter mask
            m0 = (rng.random(n) < 0.7).astype(np.uint8)
            idx.set_filter(m0)
            idx.filter_column(cols[0], op, val, validity=bm, validity_offset=off, combine=True)
            check_mask_readback(idx, oracle, X, q, oracle.and_bytes(m0, first), ctx + " AND set_filter")
            # a bitmap on both links of the chain (the second link at another offset)
            idx.filter_column(cols[1], op2, val2, validity=bm2, validity_offset=off2)
            idx.filter_column(cols[0], op, val, validity=bm, validity_offset=off, combine=True)
            both = oracle.and_bytes(rc.predicate(cols[1], val2, op2, valid2), first)
            check_mask_readback(idx, oracle, X, q, both, ctx + f" AND (op {op2} value {val2!r} offset {off2})")
    finally:
        idx.Close()


def test_negative_validity_offset_is_refused(oracle, small):
    gpu_or_skip()
    X, q = small
    n = 2000
    rng = np.random.default_rng(3)
    idx = new_index(8, L2)
    try:
        idx.Add(None, X[:n])
        mask = (rng.random(n) < 0.4).astype(np.uint8)
        idx.set_filter(mask)
        before = idx.SearchBatch(q, 2048)
        ci, cf = rc.int64_edge_column(n), rc.float32_edge_column(n)
        bm = rc.validity_bitmap(np.ones(n, bool), 8)
        lib = idx._lib
        for combine in (0, 1):
            assert lib.lb_gpu_index_filter_int64(idx._h, ci.ctypes.data, n, 0, rc.GE, bm.ctypes.data, -1, combine) == LB_ERR_INVALID_ARG
            assert lib.lb_gpu_index_filter_float32(idx._h, cf.ctypes.data, n, 0.0, rc.GE, bm.ctypes.data, -1, combine) == LB_ERR_INVALID_ARG
        after = idx.SearchBatch(q, 2048)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        check_mask_readback(idx, oracle, X, q, mask, "view after the refused calls")
    finally:
        idx.Close()


# ---- section 4: mask bytes, the 95 % switch, structured masks -------------------------------------------------------
@pytest.mark.parametrize("fraction", [0.5, 0.98])
def test_any_nonzero_mask_byte_is_visible(oracle, corpus, fraction):
    """bytes 0, 1, 2, 0x80, 0xff: the compaction (row list, 50 %) and the kernels' per-row test (98 %) both read `byte != 0`"""
    gpu_or_skip()
    X, Q = corpus
    n = X.shape[0]
    mask = rc.byte_mask(np.random.default_rng(int(fraction * 100)), n, fraction)
    assert rc.takes_row_list(int((mask != 0).sum()), n) == (fraction == 0.5)
    idx = new_index(32, L2)
    try:
        idx.Add(None, X)
        idx.set_filter(mask)
        for nq in (1, 40):
            check_lists(idx, oracle, L2, Q[:nq], X, 10, mask, f"fraction {fraction} nq {nq}")
        lab, _ = idx.SearchBatch(Q[:40], 10)
        assert np.all(mask[lab] != 0)
    finally:
        idx.Close()


@pytest.mark.parametrize("n", [2000, 20000])
def test_both_sides_of_the_list_mask_switch(oracle, corpus, n):
    """n_visible * 100 <= n * 95 walks the row list, one more visible row takes the per-row mask test: each side equals the
    oracle, and the two agree on the rows they share"""
    gpu_or_skip()
    X, Q = corpus
    X = X[:n]
    nv = n * 95 // 100
    extra = n // 7  # visible on the mask side only, and query 0's nearest neighbour there
    Q = Q[:40].copy()
    Q[0] = X[extra]
    on_list = rc.exact_count_mask(np.random.default_rng(n), n, nv, hidden=[extra])
    on_mask = on_list.copy()
    on_mask[extra] = 1
    assert on_list.sum() == nv and on_mask.sum() == nv + 1
    assert rc.takes_row_list(nv, n) and not rc.takes_row_list(nv + 1, n)
    idx = new_index(32, L2)
    try:
        idx.Add(None, X)
        for nq in (1, 40):
            idx.set_filter(on_list)
            la, da = check_lists(idx, oracle, L2, Q[:nq], X, 10, on_list, f"n {n} list side nq {nq}")
            idx.set_filter(on_mask)
            lb, db = check_lists(idx, oracle, L2, Q[:nq], X, 10, on_mask, f"n {n} mask side nq {nq}")
            assert lb[0, 0] == extra
            for q in range(nq):
                keep = lb[q] != extra
                m = int(keep.sum())
                assert np.array_equal(lb[q][keep], la[q][:m]) and np.array_equal(db[q][keep], da[q][:m]), (n, nq, q)
    finally:
        idx.Close()


@pytest.mark.parametrize("metric", [L2, COS, DOT])
def test_structured_masks(oracle, corpus, metric):
    gpu_or_skip()
    X, Q = corpus
    n, k = X.shape[0], 10
    masks = rc.structured_masks(n, k, np.random.default_rng(7))
    idx = new_index(32, metric)
    try:
        idx.Add(None, X)
        for name, mask in masks.items():
            idx.set_filter(mask)
            for nq in (1, 40):
                lab, _ = check_lists(idx, oracle, metric, Q[:nq], X, k, mask, f"metric {metric} mask '{name}' nq {nq}")
                assert np.all(mask[lab[lab >= 0]] == 1)
    finally:
        idx.Close()


# ---- section 5: the view across calls -------------------------------------------------------------------------------
@pytest.mark.parametrize("fraction", [0.5, 0.98])
def test_filter_then_add_grows_and_keeps_the_mask(oracle, corpus, fraction):
    """5000 rows, a mask, then 3000 more without reserve(): the side arrays are reallocated (capacity 5000 -> 10000), the old
    rows keep their mask bytes -- non-0/1 ones included -- and the new rows are visible"""
    gpu_or_skip()
    X, Q = corpus
    n0, n1 = 5000, 8000
    mask = rc.byte_mask(np.random.default_rng(int(fraction * 100) + 1), n0, fraction)
    idx = new_index(32, L2)
    try:
        idx.Add(None, X[:n0])
        idx.set_filter(mask)
        check_lists(idx, oracle, L2, Q[:40], X[:n0], 10, mask, "before Add")
        idx.Add(None, X[n0:n1])
        assert idx.ntotal == n1
        grown = np.concatenate([mask, np.ones(n1 - n0, np.uint8)])
        for nq in (1, 40):
            check_lists(idx, oracle, L2, Q[:nq], X[:n1], 10, grown, f"after Add, fraction {fraction} nq {nq}")
        # an AND chain over the grown mask: the new rows and the last few old ones.  (The chain is simd.AndBytes, bitwise:
        # an old byte 2 or 0x80 ANDed with a match's 1 is 0 -- the reference's result for such bytes, and the oracle's.)
        col = np.arange(n1, dtype=np.int64)
        idx.filter_column(col, ">=", n0 - 40, combine=True)
        tail = oracle.and_bytes(grown, rc.predicate(col, n0 - 40, rc.GE))
        assert 0 < np.count_nonzero(tail[:n0]) < np.count_nonzero(grown[n0 - 40:n0])
        for nq in (1, 40):
            check_lists(idx, oracle, L2, Q[:nq], X[:n1], 10, tail, f"new rows AND old bytes, fraction {fraction} nq {nq}")
    finally:
        idx.Close()


def test_combine_after_clearing_replaces(oracle, small):
    """set_filter(M1), set_filter(None), filter_column(combine=True): the predicate alone, not ANDed with M1's stale bytes"""
    gpu_or_skip()
    X, q = small
    n = 2001
    rng = np.random.default_rng(4)
    col = rng.permutation(rc.float32_edge_column(n))
    pred = rc.predicate(col, 0.25, rc.LT)
    m1 = (1 - pred).astype(np.uint8)  # ANDed in, nothing would be left
    m1[:50] = 1
    assert 0 < pred.sum() < n and oracle.and_bytes(m1, pred).sum() < pred.sum()
    idx = new_index(8, L2)
    try:
        idx.Add(None, X[:n])
        idx.set_filter(m1)
        check_mask_readback(idx, oracle, X, q, m1, "M1")
        idx.set_filter(None)
        check_mask_readback(idx, oracle, X, q, np.ones(n, np.uint8), "cleared")
        idx.filter_column(col, "<", 0.25, combine=True)
        check_mask_readback(idx, oracle, X, q, pred, "predicate after clearing")
    finally:
        idx.Close()


@pytest.mark.parametrize("how", ["set_filter", "filter_int64", "filter_float32"])
def test_filter_on_an_empty_index_then_add(oracle, small, how):
    gpu_or_skip()
    X, q = small
    n = 2000
    idx = new_index(8, L2)
    try:
        if how == "set_filter":
            idx.set_filter(np.zeros(0, np.uint8))
        else:
            idx.filter_column(np.zeros(0, np.int64 if how == "filter_int64" else F), "<", 0)
        lab, dist = idx.SearchBatch(q, 5)
        assert np.all(lab == -1) and np.all(dist == FLT_MAX)
        idx.Add(None, X[:n])
        check_mask_readback(idx, oracle, X, q, np.ones(n, np.uint8), f"{how} on the empty index, then Add")
        idx.Add(None, X[n:n + 48])
        check_mask_readback(idx, oracle, X, q, np.ones(n + 48, np.uint8), f"{how}: second Add")
    finally:
        idx.Close()


def test_wrong_length_filters_leave_the_view(oracle, small):
    gpu_or_skip()
    from longbow_amd import gpu
    X, q = small
    n = 2000
    rng = np.random.default_rng(6)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    idx = new_index(8, L2)
    try:
        idx.Add(None, X[:n])
        idx.set_filter(mask)
        before = idx.SearchBatch(q, 2048)
        for bad in (n - 1, n + 1):
            with pytest.raises(gpu.LongbowGPUError) as e:
                idx.set_filter(np.zeros(bad, np.uint8))
            assert e.value.code == LB_ERR_INVALID_ARG
            for col in (np.zeros(bad, np.int64), np.zeros(bad, F)):
                for combine in (False, True):
                    with pytest.raises(gpu.LongbowGPUError) as e:
                        idx.filter_column(col, "==", 0, combine=combine)
                    assert e.value.code == LB_ERR_INVALID_ARG
        after = idx.SearchBatch(q, 2048)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        check_mask_readback(idx, oracle, X, q, mask, "view after the refused calls")
    finally:
        idx.Close()


# ---- section 6: every route that reads a view -----------------------------------------------------------------------
def route_masks(n):
    """two masks that make the routes walk a row list, and one (98 % visible, bytes 1 / 2 / 0x80 / 0xff) that makes their
    kernels test the mask byte of every row"""
    return {"last partial block": rc.structured_masks(n, 10, np.random.default_rng(7))["last partial block"],
            "random 50 %": (np.random.default_rng(8).random(n) < 0.5).astype(np.uint8),
            "98 % of any non-zero byte": rc.byte_mask(np.random.default_rng(9), n, 0.98)}


# (mode, batch size, kinds of idx.last_route -- choose_route in index_search.hip)
ROUTES = [
    ("exact scan", CAND_AUTO, 3, (0,)),
    ("narrow 32", CAND_AUTO, 20, (1,)),
    ("narrow 64", CAND_AUTO, 100, (2,)),
    # (200 queries: the cost model prefers four 64-query tiles to one 256-query tile at 32 dimensions even in this mode;
    # beyond LB_NARROW_MAXQ = 384 queries the mode offers nothing but the tall tile)
    ("split tall tile", CAND_SPLIT_INREG, 385, (5,)),
    ("f32 wide tile", CAND_F32_MFMA, 385, (4,)),
    ("fp16 tiles, 100 queries", CAND_F16, 100, (6, 7)),
    ("fp16 tiles, 300 queries", CAND_F16, 300, (6, 7)),
]


@pytest.mark.parametrize("metric", [L2, DOT])
def test_every_route_reads_the_view(oracle, corpus, metric):
    gpu_or_skip()
    X, Q = corpus
    idx = new_index(32, metric)
    seen = {}
    try:
        idx.Add(None, X)
        for mname, mask in route_masks(X.shape[0]).items():
            idx.set_filter(mask)
            for rname, mode, nq, kinds in ROUTES:
                idx.set_candidate_mode(mode)
                ctx = f"metric {metric} mask '{mname}' route '{rname}'"
                check_lists(idx, oracle, metric, Q[:nq], X, 10, mask, ctx)
                seen[(mname, rname)] = idx.last_route[:2]
                assert idx.last_route[0] in kinds, f"{ctx}: took {idx.last_route}"
        print(f"routes, metric {metric}: {seen}")
    finally:
        idx.Close()


def test_views_on_an_fp16_index(oracle, corpus):
    gpu_or_skip()
    from longbow_amd import gpu
    X, Q = corpus
    Xh, Qh = X.astype(np.float16), Q[:40].astype(np.float16)
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=32, Metric=L2, DataType=gpu.DataType.Float16))
    try:
        idx.Add(None, Xh)
        for mname, mask in route_masks(X.shape[0]).items():
            idx.set_filter(mask)
            for nq in (3, 40):  # (an fp16 index's default order is the reference's F16 one: the 4-accumulator order)
                check_lists(idx, oracle, L2, Qh[:nq], Xh, 10, mask, f"fp16 index, mask '{mname}' nq {nq}", order=oracle.UNROLL4)
    finally:
        idx.Close()


def test_views_on_an_int8_index(corpus):
    gpu_or_skip()
    from longbow_amd import gpu
    from tests import i8_oracle as io
    X, Q = corpus
    X8 = np.floor(X * 256 - 128).astype(np.int8)
    Q8 = np.floor(Q[:40] * 256 - 128).astype(np.int8)
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=32, Metric=L2, DataType=gpu.DataType.Int8))
    try:
        idx.Add(None, X8)
        for mname, mask in route_masks(X.shape[0]).items():
            idx.set_filter(mask)
            for nq in (3, 40):
                lab, dist = idx.SearchBatch(Q8[:nq], 10)
                oi, od = io.search(L2, Q8[:nq], X8, 10, visible=np.flatnonzero(mask != 0))
                assert_same(lab, dist, oi, od, f"int8 index, mask '{mname}' nq {nq}")
    finally:
        idx.Close()
