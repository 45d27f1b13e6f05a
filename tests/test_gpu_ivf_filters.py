"""Row filters on the IVF-Flat handle (lb_gpu_ivf_set_filter, _filter_int64 / _float32, _nvisible) on the GPU.  The expected result
everywhere is tests/ivf_filter_cases.py's search_filtered (the IVF oracle over the lists with the hidden rows taken out, pinned on
the CPU by tests/test_ivf_filter_semantics.py together with the shapes of the masks below); labels and distances are compared
for equality, and lb_gpu_ivf_last_search_stats shows that a search walked the visible rows alone.  The shapes are the smallest at
which the build of the visible lists and the search sized by them can go wrong: lists emptied by the mask, visible lengths around
the scan's 128-row tile and the selection's 16,384 LDS keys, several compaction workgroups, more lists than rows, a capacity that
changes under an active filter."""
import numpy as np
import pytest

from tests import ivf_filter_cases as fc
from tests import ivf_oracle as io
from tests import row_view_cases as rv
from tests.gpu_util import assert_same, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED = 1, 6
K = fc.K


def _handle(X, C_, metric=0, order=0, ids=None):
    from longbow_amd import ivf
    gpu_or_skip()
    h = ivf.IVFFlat(C_, metric, order)
    if X.shape[0]:
        h.add(X, ids)
    return h


def _check(oracle, h, metric, order, Q, X, C_, lists, mask, k, nprobe, ids=None, ctx=""):
    """nvisible, labels, distances and the counters of a search under `mask` against the helper -> visible rows scanned"""
    ol, od, scanned = fc.search_filtered(oracle, metric, order, Q, X, C_, lists, mask, k, nprobe, ids=ids)
    assert h.nvisible() == np.count_nonzero(mask), ctx
    lab, dist = h.search(Q, k, nprobe)
    assert_same(lab, dist, ol, od, ctx)
    st = h.last_search_stats()
    assert st[:3] == (Q.shape[0], int(scanned.sum()), int(scanned.max())), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= fc.LDS_KEYS).sum()), (st, ctx)
    return scanned


@pytest.fixture(scope="module")
def parity(oracle):
    X, Q, C_ = io.parity_case()
    return X, Q, C_, io.assign(oracle, 0, 0, X, C_)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,order", [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)])
def test_parity_under_every_mask(oracle, metric, order):
    X, Q, C_ = io.parity_case()
    lists = io.assign(oracle, metric, order, X, C_)
    h = _handle(X, C_, metric, order)
    masks = fc.parity_masks()
    names = list(masks) if (metric, order) == (0, 0) else ["10 % byte mask", "50 % byte mask"]
    for name in names:
        h.set_filter(masks[name])
        assert h.ntotal == X.shape[0]
        for nprobe in (1, 3, 16):
            _check(oracle, h, metric, order, Q, X, C_, lists, masks[name], K, nprobe, ctx=f"{name}, metric {metric} order {order} nprobe {nprobe}")
    # what addresses the lists themselves ignores the filter
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_every_list_probed_equals_the_filtered_flat_index(metric):
    X, Q, C_ = io.parity_case()
    mask = fc.parity_masks()["10 % byte mask"]
    for order in (0, 1):
        h = _handle(X, C_, metric, order)
        h.set_filter(mask)
        flat = new_index(X.shape[1], metric, order)
        flat.Add(None, X)
        flat.set_filter(mask)
        fl, fd = flat.SearchBatch(Q, K)
        for nprobe in (16, 21):
            lab, dist = h.search(Q, K, nprobe)
            assert_same(lab, dist, fl, fd, f"metric {metric} order {order} nprobe {nprobe}")
            assert h.last_search_stats()[1] == Q.shape[0] * np.count_nonzero(mask)
        flat.Close()
        h.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("choice", ["first rows", "random rows"])
def test_visible_list_lengths_at_the_tile_edges(oracle, choice):
    X, Q, C_, owner = io.edge_case(fc.EDGE_COUNTS)
    mask = fc.keep_per_list(owner, fc.EDGE_KEEP, None if choice == "first rows" else np.random.default_rng(6))
    h = _handle(X, C_)
    assert h.list_sizes().tolist() == list(fc.EDGE_COUNTS)
    h.set_filter(mask)
    assert h.list_sizes().tolist() == list(fc.EDGE_COUNTS)
    for nprobe in (1, 2):
        for k in (10, 200):
            scanned = _check(oracle, h, 0, 0, Q, X, C_, owner, mask, k, nprobe, ctx=f"{choice} nprobe {nprobe} k {k}")
            if nprobe == 1:
                assert scanned.tolist() == list(fc.EDGE_KEEP)
    lab, dist = h.search(Q, 10, 1)
    assert (lab[0] == -1).all() and (dist[0] == io.FLT_MAX).all()  # a probed list with no visible row: all padding
    assert lab[1, 0] == np.flatnonzero((owner == 1) & (mask != 0))[0] and (lab[1, 1:] == -1).all() and (dist[1, 1:] == io.FLT_MAX).all()
    h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_the_selection_follows_the_visible_count(oracle):
    """50,000 rows: 25 compaction workgroups and 13 sort chunks.  List 0 holds about 37,000 rows, more than any selection from
    LDS takes; with exactly 16,384 of them visible the three queries that probe it are selected from LDS, with one more not."""
    X, Q, C_ = io.skew_case()
    lists = io.assign(oracle, 0, 0, X, C_)
    h = _handle(X, C_)
    for keep0, from_lds in ((fc.LDS_KEYS, 5), (fc.LDS_KEYS + 1, 2)):
        mask = fc.skew_mask(lists, keep0)
        h.set_filter(mask)
        for k in (1, 100, 2048):
            _check(oracle, h, 0, 0, Q, X, C_, lists, mask, k, 1, ctx=f"{keep0} visible in list 0, k {k}")
            assert h.last_search_stats()[3] == from_lds
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_more_lists_than_rows(oracle):
    from longbow_amd import _lib
    X, Q, _ = io.parity_case(nq=9)
    C_ = np.random.default_rng(55).standard_normal((4096, X.shape[1])).astype(F)
    lists = io.assign(oracle, 0, 0, X, C_)
    mask = fc.parity_masks()["10 % byte mask"]
    h = _handle(X, C_)
    assert np.array_equal(h.assignments(), lists)
    # 4096 probes are more than the coarse search returns (LB_MAX_K): every list probed takes all lists without it, filter or none
    ol, od, _ = io.search(oracle, 0, 0, Q, X, C_, lists, K, 4096)
    assert_same(*h.search(Q, K, 4096), ol, od, "4096 lists, every list probed, no filter")
    with pytest.raises(_lib.LongbowGPUError) as e:
        h.search(Q, K, 4095)
    assert e.value.code == UNSUPPORTED
    h.set_filter(mask)
    for nprobe in (1, 64, 4096):
        _check(oracle, h, 0, 0, Q, X, C_, lists, mask, K, nprobe, ctx=f"4096 lists, nprobe {nprobe}")
    h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_filter_column_equals_set_filter_of_the_restated_predicate(oracle, parity):
    X, Q, C_, lists = parity
    n = X.shape[0]
    rng = np.random.default_rng(17)
    cols = {"int64": (rv.int64_edge_column(n), 2 ** 32), "float32": (rv.float32_edge_column(n), 0.25)}
    valid = rng.random(n) < 0.8
    byte_mask = fc.parity_masks()["50 % byte mask"]
    h, twin = _handle(X, C_), _handle(X, C_)

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
    _check(oracle, h, 0, 0, Q, X, C_, lists, m2, K, 3, ctx="combined, against the helper")
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
    the handle past them (3000 -> 5000 rows) under the active filter"""
    X, Q, C_, lists = parity
    rng = np.random.default_rng(7)
    more = rng.standard_normal((2000, X.shape[1])).astype(F)
    all_rows = np.concatenate([X, more])
    all_lists = np.concatenate([lists, io.assign(oracle, 0, 0, more, C_)])
    ids = rng.permutation(1 << 20)[:all_rows.shape[0]].astype(np.int64) + (1 << 41) if with_ids else None
    sub = lambda a, b: None if ids is None else ids[a:b]
    mask = rv.byte_mask(rng, 1000, 0.5)
    h = _handle(X[:1000], C_, ids=sub(0, 1000))
    h.set_filter(mask)
    before = h.hbm_bytes
    for n in (3000, 5000):
        h.add(all_rows[h.ntotal:n], sub(h.ntotal, n))
        full = np.concatenate([mask, np.ones(n - 1000, np.uint8)])
        assert h.ntotal == n and np.array_equal(h.assignments(), all_lists[:n])
        assert np.array_equal(h.list_sizes(), np.bincount(all_lists[:n], minlength=C_.shape[0]))
        for nprobe in (3, 16):
            _check(oracle, h, 0, 0, Q, all_rows[:n], C_, all_lists[:n], full, K, nprobe, ids=sub(0, n), ctx=f"{n} rows nprobe {nprobe}")
    assert h.hbm_bytes > before
    h.reserve(20000)  # a change of capacity alone keeps the filter too
    _check(oracle, h, 0, 0, Q, all_rows, C_, all_lists, full, K, 3, ids=ids, ctx="after reserve")
    h.Close()


def test_a_filter_set_on_an_empty_handle_covers_what_is_added(oracle, parity):
    X, Q, C_, lists = parity
    h = _handle(X[:0], C_)
    h.set_filter(np.zeros(0, np.uint8))
    assert h.nvisible() == 0
    lab, dist = h.search(Q, K, 3)
    assert (lab == -1).all() and (dist == io.FLT_MAX).all() and h.last_search_stats() == (Q.shape[0], 0, 0, 0)
    h.add(X[:300])
    assert h.nvisible() == 300
    _check(oracle, h, 0, 0, Q, X[:300], C_, lists[:300], np.ones(300, np.uint8), K, 3, ctx="filter set on an empty handle")
    h.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_replace_and_clear(oracle, parity):
    X, Q, C_, lists = parity
    masks = fc.parity_masks()
    h, twin = _handle(X, C_), _handle(X, C_)
    assert h.nvisible() == X.shape[0]
    h.set_filter(masks["10 % byte mask"])
    _check(oracle, h, 0, 0, Q, X, C_, lists, masks["10 % byte mask"], K, 3, ctx="first mask")
    h.set_filter(masks["50 % byte mask"])
    _check(oracle, h, 0, 0, Q, X, C_, lists, masks["50 % byte mask"], K, 3, ctx="second mask")
    h.set_filter(None)
    assert h.nvisible() == h.ntotal == X.shape[0]
    for nprobe in (1, 3, 16):
        assert_same(*h.search(Q, K, nprobe), *twin.search(Q, K, nprobe), f"cleared, nprobe {nprobe}")
        assert h.last_search_stats() == twin.last_search_stats()
    h.Close()
    twin.Close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_behind_a_live_handle(oracle, parity):
    from longbow_amd import _lib
    X, Q, C_, lists = parity
    n = X.shape[0]
    mask = fc.parity_masks()["50 % byte mask"]
    h = _handle(X, C_)
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
    assert lib.lb_gpu_ivf_filter_int64(h._h, col.ctypes.data, n, 0, 6, None, 0, 0) == INVALID
    assert lib.lb_gpu_ivf_filter_int64(h._h, col.ctypes.data, n, 0, -1, None, 0, 0) == INVALID
    assert lib.lb_gpu_ivf_filter_int64(h._h, col.ctypes.data, n, 0, 0, valid.ctypes.data, -1, 0) == INVALID
    assert lib.lb_gpu_ivf_filter_float32(h._h, col.ctypes.data, n, 0.0, 6, None, 0, 1) == INVALID
    assert h.nvisible() == np.count_nonzero(mask)
    assert_same(*h.search(Q, K, 3), *want, "after a refused op")
    h.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [5, 768])
def test_other_scan_forms_under_a_filter(oracle, dim):
    """5: the one-lane-per-row form; 768: twelve chunks of the staged form"""
    n, nlist, nprobe, k, nq = (3000, 16, 4, 100, 3) if dim == 768 else (1000, 7, 2, 10, 9)
    X, Q, C_ = io.parity_case(n, dim, nlist, nq, seed=dim)
    mask = rv.byte_mask(np.random.default_rng(dim), n, 0.5)
    for metric, order in ((0, 0), (1, 1)):
        lists = io.assign(oracle, metric, order, X, C_)
        h = _handle(X, C_, metric, order)
        h.set_filter(mask)
        _check(oracle, h, metric, order, Q, X, C_, lists, mask, k, nprobe, ctx=f"dim {dim} metric {metric} order {order}")
        h.Close()


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_python_mirror(oracle, parity):
    from longbow_amd import ivf
    X, Q, C_, lists = parity
    n = X.shape[0]
    idx = ivf.IVFFlatIndex(X.shape[1], ivf.IVFFlatConfig(NClusters=16, NProbe=3), centroids=C_)
    idx.AddBatch(np.arange(n), X)
    for call in (lambda: idx.set_filter(np.ones(n, np.uint8)), lambda: idx.filter_column(np.zeros(n, np.int64), 0, rv.EQ), idx.nvisible):
        with pytest.raises(RuntimeError):
            call()
    idx.Build()
    assert idx.nvisible() == n
    col = rv.int64_edge_column(n)
    idx.filter_column(col, 5, ">=")
    mask = rv.predicate(col, 5, rv.GE)
    assert 0 < mask.sum() < n and idx.nvisible() == mask.sum()
    ol, od, _ = fc.search_filtered(oracle, 0, 0, Q, X, C_, lists, mask, K, 3)
    assert_same(*idx.SearchBatch(Q, K), ol, od, "SearchBatch under filter_column")
    idx.set_filter(None)
    assert idx.nvisible() == n
    idx.Close()
