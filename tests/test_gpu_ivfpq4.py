"""lb_gpu_ivfpq4_* on the GPU against the C oracle, bit for bit on labels and distances, plain and residual: the lists and the
probes are tests/ivf_oracle.py's, the codes oracle.pq_encode's K <= 16 branch (over row - C[list] for a residual handle), the table
oracle.build_adc_table at stride 16 (over q - C[list] per probed list for a residual handle), the row sums oracle.adc_single
under float32(sqrt(float64(s))) as tests/test_gpu_pq4.py, the result a stable sort on (distance, row).  The inputs are
tests/ivfpq_oracle.py's with their codebooks cut to 16 centroids; 4-bit codes tie often, so the row order is exercised."""
import numpy as np
import pytest

from tests import ivf_oracle as io
from tests import ivfpq_oracle as pqo
from tests import ivfpq_residual_oracle as ro
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
UNSUPPORTED = 6
LDS_KEYS = 16384  # IVF_SELECT_LDS_KEYS
BOTH = pytest.mark.parametrize("residual", [False, True])


def _handle(X, C_, cb, order=0, residual=False):
    from longbow_amd import ivfpq4
    gpu_or_skip()
    h = ivfpq4.IVFPQ4(pqo.blob(cb), C_, order, residual=residual)
    assert h.residual is residual and h.m == cb.shape[0]
    h.add(X)
    return h


def _ref_codes(oracle, cb, X, C_, lists, residual):
    return pqo.encode(oracle, cb, ro.residuals(X, C_, lists) if residual else X)


def _ref_search(oracle, cb, order, Q, C_, lists, codes, k, nprobe, residual, visible=None):
    """-> (labels [nq, k], dist [nq, k], rows scanned per query [nq]); visible: a mask over the rows (a hidden row is in no list)"""
    lists = np.asarray(lists) if visible is None else np.where(np.asarray(visible) != 0, lists, -1)
    labels = np.full((Q.shape[0], k), -1, np.int64)
    dist = np.full((Q.shape[0], k), pqo.FLT_MAX, F)
    scanned = np.empty(Q.shape[0], np.int64)
    for j in range(Q.shape[0]):
        pr = io.probes(oracle, 0, order, Q[j], C_, nprobe)
        rows = io.probed_rows(lists, pr)
        scanned[j] = rows.size
        d = np.empty(rows.size, F)
        for l in (pr if residual else [None]):  # a residual handle: a table per probed list
            sel = lists[rows] == l if residual else np.ones(rows.size, bool)
            if sel.any():
                table = oracle.build_adc_table(cb, (Q[j] - C_[l]).astype(F) if residual else Q[j])
                uniq, inv = np.unique(codes[rows[sel]], axis=0, return_inverse=True)  # (equal code rows: one sum)
                s = np.array([oracle.adc_single(table, c, 16) for c in uniq], F)
                d[sel] = np.sqrt(s.astype(np.float64)).astype(F)[inv.reshape(-1)]
        o = np.argsort(d, kind="stable")[:k]  # rows ascend: ascending (distance, row)
        labels[j, :o.size], dist[j, :o.size] = rows[o], d[o]
    return labels, dist, scanned


def _check(oracle, h, cb, order, Q, C_, lists, codes, k, nprobe, visible=None, ctx=""):
    ol, od, scanned = _ref_search(oracle, cb, order, Q, C_, lists, codes, k, nprobe, h.residual, visible)
    assert_same(*h.search(Q, k, nprobe), ol, od, ctx)
    st = h.last_search_stats()
    assert st == (Q.shape[0], int(scanned.sum()), int(scanned.max()), int((scanned <= LDS_KEYS).sum())), (st, ctx)
    return ol, od


# 1: the row forms -- odd M in single bytes with a spare nibble, P = 16, the workload's P = 48, run-time P = 80, P = 17 -----------
@BOTH
@pytest.mark.parametrize("dims,M,order", [(6, 3, 0), (64, 32, 0), (192, 96, 0), (192, 96, 1), (320, 160, 0), (68, 34, 0)])
def test_row_forms(oracle, dims, M, order, residual):
    from longbow_amd import pq4
    X, Q, C_, cb = pqo.parity_case(dims, M)
    cb = np.ascontiguousarray(cb[:, :16])
    lists = pqo.assign(oracle, order, X, C_)
    codes = _ref_codes(oracle, cb, X, C_, lists, residual)
    h = _handle(X, C_, cb, order, residual)
    assert h.ntotal == X.shape[0] and np.array_equal(h.assignments(), lists)
    assert np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    assert np.array_equal(h.codes(), codes) and np.array_equal(h.codes(100, 7), codes[100:107])
    for nprobe in (1, 3, 16):
        got = _check(oracle, h, cb, order, Q, C_, lists, codes, 10, nprobe, ctx=f"nprobe {nprobe}")
    if not residual:  # every list probed: the flat PQ4 handle over the same codes
        enc = pq4.PQ4Encoder(pqo.blob(cb))
        enc.add_codes(h.codes())
        assert_same(*enc.Search(Q, 10), *got, "against pq4.PQ4Encoder.Search")
        enc.Close()
    h.Close()


# 2: list lengths around the tile, and both shapes of the residual scan -----------------------------------------------------------
@pytest.fixture(scope="module")
def edge(oracle):
    X, Q, C_, owner, cb = pqo.edge_case()
    cb = np.ascontiguousarray(cb[:, :16])
    return X, Q, C_, owner, cb, {r: _ref_codes(oracle, cb, X, C_, owner, r) for r in (False, True)}


@BOTH
@pytest.mark.parametrize("nprobe,k", [(1, 10), (1, 200), (2, 10), (len(pqo.EDGE_COUNTS), 200)])
def test_list_lengths(oracle, edge, nprobe, k, residual):
    """The residual scan's launch shape for these numbers, by the plan function restated in tests/ivfpq_residual_oracle.py: the 66
    queries at one probe are 66 pairs of 8 workgroups, and the longest list (8 * 1024 + 77 rows, 9 tiles) takes their second
    stride step; at two probes (132 pairs of 4 workgroups: 9 tiles > 2 * 4) and at every list the scan runs from the work list."""
    X, Q, C_, owner, cb, codes = edge
    sizes = np.sort(np.array(pqo.EDGE_COUNTS))[::-1]
    plan = ro.rscan_plan(Q.shape[0] * nprobe, Q.shape[0], int(sizes[:nprobe].sum()), int(sizes[0]))
    assert plan[0] == ("strided" if nprobe == 1 else "items") and (nprobe > 1 or plan[1] == 8)
    h = _handle(X, C_, cb, residual=residual)
    assert np.array_equal(h.assignments(), owner) and np.array_equal(h.codes(), codes[residual])
    lab, dist = _check(oracle, h, cb, 0, Q, C_, owner, codes[residual], k, nprobe)
    if nprobe == 1:
        assert (lab[0] == -1).all() and (dist[0] == pqo.FLT_MAX).all()  # an empty probed list: all padding
    h.Close()


# 3: selection beyond LDS ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skew(oracle):
    X, Q, C_, cb = pqo.skew_case()
    cb = np.ascontiguousarray(cb[:, :16])
    lists = pqo.assign(oracle, 0, X, C_)
    return X, Q, C_, cb, lists, {r: _ref_codes(oracle, cb, X, C_, lists, r) for r in (False, True)}


@BOTH
@pytest.mark.parametrize("nprobe,from_lds", [(1, 2), (4, 0)])  # from_lds: what the K = 256 handle reports at these inputs
@pytest.mark.parametrize("k", [1, 2048])
def test_selection_beyond_lds(oracle, skew, k, nprobe, from_lds, residual):
    X, Q, C_, cb, lists, codes = skew
    h = _handle(X, C_, cb, residual=residual)
    _check(oracle, h, cb, 0, Q, C_, lists, codes[residual], k, nprobe)
    assert h.last_search_stats()[3] == from_lds
    h.Close()


# 4: more pairs than one batch's table budget holds ----------------------------------------------------------------------------------
def test_batches_by_the_table_budget(oracle):
    """M = 1024: a table is 64 KB (what the K = 256 rule gives 64 subspaces), so 1 GiB holds 16,384 tables: 126 queries at 130
    probes.  130 queries run as two batches; the oracle checks the queries across the first batch's end."""
    dims = M = 1024
    nlist, nq = 130, 130
    assert ro.table_plan(nlist, M // 16) == (126, nlist)
    X, Q, C_, cb = pqo.parity_case(dims, M, n=500, nlist=nlist, nq=nq)
    cb = np.ascontiguousarray(cb[:, :16])
    lists = pqo.assign(oracle, 0, X, C_)
    codes = _ref_codes(oracle, cb, X, C_, lists, True)
    h = _handle(X, C_, cb, residual=True)
    assert np.array_equal(h.codes(), codes)
    lab, dist = h.search(Q, 10, nlist)
    assert h.last_search_stats()[:3] == (nq, nq * 500, 500)
    ol, od, _ = _ref_search(oracle, cb, 0, Q[122:130], C_, lists, codes, 10, nlist, True)
    assert_same(lab[122:130], dist[122:130], ol, od, "across the first batch's end")
    assert_same(*h.search(Q[126:], 10, nlist), lab[126:], dist[126:], "the second batch alone")
    h.Close()


# 5: visibility -- a filter, the same mask as a call bitmap, removal, compaction -------------------------------------------------------
@BOTH
def test_filter_bitmap_removal_and_compaction(oracle, residual):
    from longbow_amd import ivfpq4
    dims, M = 68, 34  # P = 17: the list-major copy and the compaction move rows of an odd width
    X, Q, C_, cb = pqo.parity_case(dims, M)
    cb = np.ascontiguousarray(cb[:, :16])
    n, nlist = X.shape[0], C_.shape[0]
    lists = pqo.assign(oracle, 0, X, C_)
    codes = _ref_codes(oracle, cb, X, C_, lists, residual)
    mask = (np.random.default_rng(34).random(n) < 0.3).astype(np.uint8)
    bits, stride = ivfpq4.pack_bitmap(mask)
    h = _handle(X, C_, cb, residual=residual)
    for nprobe in (1, nlist):
        h.set_filter(mask)
        assert h.nvisible() == np.count_nonzero(mask)
        want = _check(oracle, h, cb, 0, Q, C_, lists, codes, 10, nprobe, visible=mask, ctx=f"filter, nprobe {nprobe}")
        stats = h.last_search_stats()
        h.set_filter(None)
        assert_same(*h.search(Q, 10, nprobe, bitmap=bits, bitmap_stride=stride), *want, f"call bitmap, nprobe {nprobe}")
        assert h.last_search_stats() == stats and h.nvisible() == n  # the handle is left as it was
    gone = np.arange(0, n, 7)
    live = np.ones(n, np.uint8)
    live[gone] = 0
    assert h.remove_rows(gone) == gone.size and h.nlive() == n - gone.size and h.ndeleted() == gone.size
    for nprobe in (1, nlist):
        _check(oracle, h, cb, 0, Q, C_, lists, codes, 10, nprobe, visible=live, ctx=f"removed, nprobe {nprobe}")
    keep = np.flatnonzero(live)
    assert np.array_equal(h.compact(), keep) and h.ntotal == keep.size and h.ndeleted() == 0
    assert np.array_equal(h.codes(), codes[keep]) and np.array_equal(h.assignments(), lists[keep])
    fresh = _handle(X[keep], C_, cb, residual=residual)
    for nprobe in (1, nlist):
        assert_same(*h.search(Q, 10, nprobe), *fresh.search(Q, 10, nprobe), f"compacted, nprobe {nprobe}")
        _check(oracle, h, cb, 0, Q, C_, lists[keep], codes[keep], 10, nprobe, ctx=f"compacted, nprobe {nprobe}")
    fresh.Close()
    h.Close()


# 6: refusals --------------------------------------------------------------------------------------------------------------------------
@BOTH
def test_refusals(residual):
    from longbow_amd import _lib, ivfpq4
    gpu_or_skip()
    rng = np.random.default_rng(6)
    C_ = rng.standard_normal((4, 8)).astype(F)
    for cb, cent in ((rng.standard_normal((4, 256, 2)).astype(F), C_),                 # a well-formed blob of another K
                     (np.zeros((1025, 16, 1), F), np.zeros((4, 1025), F))):          # M > PQ4_MAX_M
        with pytest.raises(_lib.LongbowGPUError) as e:
            ivfpq4.IVFPQ4(pqo.blob(cb), cent, residual=residual)
        assert e.value.code == UNSUPPORTED
    h = _handle(rng.standard_normal((50, 8)).astype(F), C_, rng.standard_normal((4, 16, 2)).astype(F), residual=residual)
    h.Close()
    with pytest.raises(_lib.LongbowGPUError):
        h.add(C_)
