"""The residual IVF-PQ handle (lb_gpu_ivfpq_new_residual) on the GPU against tests/ivfpq_residual_oracle.py (the residual
semantics restated over the C oracle's batch_flat, pq_encode, build_adc_table, adc_batch and topk_canonical): labels and distances
must be equal, bit for bit.  The shapes are tests/test_gpu_ivfpq.py's, the smallest at which the residual kernels can still go
wrong: the byte and the 16-byte forms of the scan, lists around the 1024-position tile, a list that needs the stride loop of its
pair's workgroups, empty slots, selections within LDS and beyond, the workload's table and the largest one, row filters, more
pairs than a batch's table budget holds, and one query whose tables go in two rounds of slots."""
import threading

import numpy as np
import pytest

from tests import ivf_oracle as io
from tests import ivf_piece_cases as pc
from tests import ivfpq_oracle as pqo
from tests import ivfpq_residual_oracle as ro
from tests import row_view_cases as rv
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED, CANCELLED = 1, 6, 8
LB_MAX_K = 2048
LDS_KEYS = 16384  # IVF_SELECT_LDS_KEYS


def _handle(X, C_, cb, order=0, ids=None, residual=True):
    from longbow_amd import ivfpq
    gpu_or_skip()
    h = ivfpq.IVFPQ(pqo.blob(cb), C_, order, residual=residual)
    assert h.residual is residual and h._lib.lb_gpu_ivfpq_residual(h._h) == int(residual)
    if X.shape[0]:
        h.add(X, ids)
    return h


def _check_search(oracle, h, cb, order, Q, C_, lists, codes, k, nprobe, ids=None, visible=None, ctx=""):
    ol, od, scanned = ro.search(oracle, cb, order, Q, C_, lists, codes, k, nprobe, ids=ids, visible=visible)
    lab, dist = h.search(Q, k, nprobe)
    assert_same(lab, dist, ol, od, ctx)
    st = h.last_search_stats()
    assert st[0] == Q.shape[0] and st[1] == int(scanned.sum()) and st[2] == int(scanned.max()), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= LDS_KEYS).sum()), (st, ctx)
    return scanned


@pytest.fixture(scope="module")
def parity(oracle):
    """the byte-form shape of case 1 with its oracle lists and residual codes at order 0"""
    X, Q, C_, cb = pqo.parity_case(*pqo.PARITY_SHAPES[0])
    lists = pqo.assign(oracle, 0, X, C_)
    return X, Q, C_, cb, lists, ro.encode(oracle, cb, X, C_, lists)


@pytest.fixture(scope="module")
def edge(oracle):
    X, Q, C_, owner, cb = pqo.edge_case()
    return X, Q, C_, owner, cb, ro.encode(oracle, cb, X, C_, owner)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dims,M", pqo.PARITY_SHAPES)
def test_parity_grid(oracle, dims, M, order):
    """the centroids are rows of the input: their residuals are zero (tests/test_ivfpq_residual_semantics.py)"""
    X, Q, C_, cb = pqo.parity_case(dims, M)
    lists = pqo.assign(oracle, order, X, C_)
    codes = ro.encode(oracle, cb, X, C_, lists)
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
def test_list_length_edges(oracle, edge):
    """tests/test_ivfpq_residual_semantics.py asserts of this input what the case needs: the counts, and the second step of the
    stride loop over the long list at nprobe = 1"""
    X, Q, C_, owner, cb, codes = edge
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


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_the_long_selection(oracle):
    X, Q, C_, cb = pqo.skew_case()
    lists = pqo.assign(oracle, 0, X, C_)
    codes = ro.encode(oracle, cb, X, C_, lists)
    h = _handle(X, C_, cb)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.codes(), codes)
    from_lds = []
    for nprobe in (1, 4):
        for k in (1, 100, 2048):
            scanned = _check_search(oracle, h, cb, 0, Q, C_, lists, codes, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
            from_lds.append(h.last_search_stats()[3])
    assert scanned.min() > LDS_KEYS
    assert from_lds == [2, 2, 2, 0, 0, 0]  # as the plain handle's: the plan and the selection are its
    h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,M,n,nlist,nprobes", [
    (192, 96, 2000, 8, (2, 8)),      # the workload's table: 98,304 B of LDS a pair
    (159, 159, 500, 130, (2, 129)),  # the largest table: 162,816 B
    (4, 1, 1000, 8, (2, 8)),
    (80, 80, 700, 8, (3,)),          # M % 16 == 0 without a compile-time form
])
def test_table_sizes(oracle, dims, M, n, nlist, nprobes):
    X, Q, C_, cb = pqo.parity_case(dims, M, n=n, nlist=nlist, nq=5)
    lists = pqo.assign(oracle, 0, X, C_)
    codes = ro.encode(oracle, cb, X, C_, lists)
    h = _handle(X, C_, cb)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.codes(), codes)
    for nprobe in nprobes:
        _check_search(oracle, h, cb, 0, Q, C_, lists, codes, 10, nprobe, ctx=f"M {M} nprobe {nprobe}")
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,M", pqo.PARITY_SHAPES)
def test_zero_centroid_equals_the_plain_handle(oracle, dims, M):
    """every row in a list whose centroid is all zeros: x - 0 = x, so a residual handle is the plain one, bit for bit"""
    X, Q, C_, cb = ro.zero_centroid_case(dims, M)
    r, p = _handle(X, C_, cb), _handle(X, C_, cb, residual=False)
    assert (r.assignments() == 0).all() and np.array_equal(r.assignments(), p.assignments())
    codes = r.codes()
    assert np.array_equal(codes, p.codes()) and np.array_equal(codes, pqo.encode(oracle, cb, X))
    for nprobe in (1, 2, 3):
        assert_same(*r.search(Q, 10, nprobe), *p.search(Q, 10, nprobe), f"nprobe {nprobe}")
        assert r.last_search_stats() == p.last_search_stats()
    _check_search(oracle, r, cb, 0, Q, C_, np.zeros(X.shape[0], np.int64), codes, 10, 3, ctx="against the residual oracle")
    r.Close()
    p.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_adds_in_pieces_with_ids(oracle, parity):
    import torch
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
        _check_search(oracle, pieces, cb, 0, Q[:5], C_, lists[:r0], codes[:r0], 10, 3, ids=ids, ctx=f"after {r0} rows")
    assert r0 == X.shape[0]
    want = one.search(Q, 10, 3)
    ol, od, _ = ro.search(oracle, cb, 0, Q, C_, lists, codes, 10, 3, ids=ids)
    assert_same(*want, ol, od, "one add, ids")
    assert_same(*pieces.search(Q, 10, 3), *want, "adds in pieces")
    assert_same(*dev.search(Q, 10, 3), *want, "device-pointer adds")
    assert np.array_equal(dev.assignments(), lists) and np.array_equal(dev.codes(), codes)
    dQ = torch.from_numpy(Q).cuda()
    dD = torch.full((Q.shape[0], 10), -5.0, dtype=torch.float32, device="cuda")
    dL = torch.full((Q.shape[0], 10), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    pieces.search_device(Q.shape[0], dQ.data_ptr(), 10, 3, dD.data_ptr(), dL.data_ptr())
    assert_same(dL.cpu().numpy(), dD.cpu().numpy(), *want, "device-pointer search")
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


# 7 ---------------------------------------------------------------------------------------------------------------------------
def _masks(n, seed):
    rng = np.random.default_rng(seed)
    one = np.zeros(n, np.uint8)
    one[n // 3] = 1
    return {"all visible": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "one row": one,
            "50 %": rv.byte_mask(rng, n, 0.5), "10 %": rv.byte_mask(rng, n, 0.1)}


def _check_filtered(oracle, h, cb, Q, C_, lists, codes, mask, k, nprobe, ctx):
    assert h.nvisible() == np.count_nonzero(mask), ctx
    return _check_search(oracle, h, cb, 0, Q, C_, lists, codes, k, nprobe, visible=mask, ctx=ctx)


def test_row_filters_on_the_parity_case(oracle, parity):
    X, Q, C_, cb, lists, codes = parity
    n = X.shape[0]
    h = _handle(X, C_, cb)
    unfiltered = {nprobe: h.search(Q, 10, nprobe) for nprobe in (1, 3, 16)}
    for name, mask in _masks(n, 31).items():
        h.set_filter(mask)
        for nprobe in (1, 3, 16):
            _check_filtered(oracle, h, cb, Q, C_, lists, codes, mask, 10, nprobe, f"{name} nprobe {nprobe}")
    col = rv.int64_edge_column(n)
    h.filter_column(col, 2 ** 32, rv.LT)
    pred = rv.predicate(col, 2 ** 32, rv.LT)
    assert 0 < np.count_nonzero(pred) < n
    for nprobe in (1, 3, 16):
        _check_filtered(oracle, h, cb, Q, C_, lists, codes, pred, 10, nprobe, f"int64 predicate nprobe {nprobe}")
    # an add under the filter: the new rows are visible, and both the codes and the results stay right
    more = np.random.default_rng(9).standard_normal((500, X.shape[1])).astype(F)
    more_lists = pqo.assign(oracle, 0, more, C_)
    all_lists = np.concatenate([lists, more_lists])
    all_codes = np.concatenate([codes, ro.encode(oracle, cb, more, C_, more_lists)])
    h.add(more)
    full = np.concatenate([pred, np.ones(500, np.uint8)])
    assert h.ntotal == n + 500 and np.array_equal(h.codes(), all_codes) and np.array_equal(h.assignments(), all_lists)
    for nprobe in (3, 16):
        _check_filtered(oracle, h, cb, Q, C_, all_lists, all_codes, full, 10, nprobe, f"after an add under the filter, nprobe {nprobe}")
    h.set_filter(None)  # cleared: the unfiltered search of all rows
    assert h.nvisible() == h.ntotal
    _check_search(oracle, h, cb, 0, Q, C_, all_lists, all_codes, 10, 3, ctx="cleared after the add")
    h.Close()
    # clearing restores the unfiltered results
    h = _handle(X, C_, cb)
    h.set_filter(_masks(n, 31)["10 %"])
    h.set_filter(None)
    for nprobe, want in unfiltered.items():
        assert_same(*h.search(Q, 10, nprobe), *want, f"cleared, nprobe {nprobe}")
    h.Close()


def test_row_filters_on_the_edge_case(oracle, edge):
    X, Q, C_, owner, cb, codes = edge
    n, nlist = X.shape[0], C_.shape[0]
    h = _handle(X, C_, cb)
    want = h.search(Q, 10, 2)
    masks = _masks(n, 32)
    col = rv.int64_edge_column(n)
    for name in list(masks) + ["int64 predicate"]:
        if name == "int64 predicate":
            h.filter_column(col, 2 ** 32, rv.GE)
            mask = rv.predicate(col, 2 ** 32, rv.GE)
        else:
            mask = masks[name]
            h.set_filter(mask)
        for nprobe, k in ((1, 10), (2, 200), (nlist, 10)):
            _check_filtered(oracle, h, cb, Q, C_, owner, codes, mask, k, nprobe, f"{name} nprobe {nprobe} k {k}")
    h.set_filter(None)
    assert_same(*h.search(Q, 10, 2), *want, "cleared")
    h.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_batches_by_the_table_budget_and_concurrent_searches(oracle):
    """M = 159, every one of 130 lists probed: 1 GiB of tables holds 50 queries' pairs (tests/test_ivfpq_residual_semantics.py
    pins the rule), so 120 queries run as three batches"""
    dims = M = 159
    nlist, nq = 130, 120
    assert ro.batch_queries(nq, nlist, M) == 50
    X, Q, C_, cb = pqo.parity_case(dims, M, n=500, nlist=nlist, nq=nq)
    lists = pqo.assign(oracle, 0, X, C_)
    codes = ro.encode(oracle, cb, X, C_, lists)
    h = _handle(X, C_, cb)
    assert np.array_equal(h.codes(), codes)
    lab, dist = h.search(Q, 10, nlist)
    assert h.last_search_stats()[:3] == (nq, nq * 500, 500)
    ol, od, _ = ro.search(oracle, cb, 0, Q[45:55], C_, lists, codes, 10, nlist)  # across the first batch's end
    assert_same(lab[45:55], dist[45:55], ol, od, "against the oracle")
    for j in range(nq):  # query by query
        l1, d1 = h.search(Q[j:j + 1], 10, nlist)
        assert_same(l1, d1, lab[j:j + 1], dist[j:j + 1], f"query {j} alone")
    out = [None] * 4

    def work(t):
        out[t] = h.search(Q[t * 20:t * 20 + 60], 10, nlist)  # two batches each

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for t in range(4):
        assert_same(*out[t], lab[t * 20:t * 20 + 60], dist[t * 20:t * 20 + 60], f"thread {t}")
    h.Close()


def test_more_queries_than_a_batch(oracle, parity):
    X, Q, C_, cb, lists, codes = parity
    big = np.random.default_rng(8).standard_normal((1025, X.shape[1])).astype(F)
    h = _handle(X, C_, cb)
    ol, od, scanned = ro.search(oracle, cb, 0, big, C_, lists, codes, 10, 3)
    for nq in (1, 1025):
        lab, dist = h.search(big[:nq], 10, 3)
        assert_same(lab, dist, ol[:nq], od[:nq], f"nq {nq}")
        assert h.last_search_stats()[:2] == (nq, int(scanned[:nq].sum()))
    h.set_profiling(True)
    assert_same(*h.search(big, 10, 3), ol, od, "profiled")
    ms = h.last_timing()
    assert len(ms) == 5 and all(np.isfinite(t) and t >= 0 for t in ms) and sum(ms) > 0, ms
    h.Close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_rounds_of_slots(oracle):
    """M = 159 and 6,600 lists, all probed: one query's tables are beyond 1 GiB, so they go in two rounds of slots (6,594 and
    6) into the one run of keys.  The only case that needs about 1 GiB of scratch: one handle, two searches."""
    dims = M = 159
    nlist, n = 6600, 8000
    assert ro.slot_rounds(nlist, M) == 2
    rng = np.random.default_rng(159)
    C_ = rng.standard_normal((nlist, dims)).astype(F)
    X = rng.standard_normal((n, dims)).astype(F)
    Q = rng.standard_normal((2, dims)).astype(F)
    cb = pqo.codebooks(dims, M, 6600)
    lists = pqo.assign(oracle, 0, X, C_)
    assert (np.bincount(lists, minlength=nlist)[6594:] > 0).any()  # the second round has rows to scan
    codes = ro.encode(oracle, cb, X, C_, lists)
    h = _handle(X, C_, cb)
    assert np.array_equal(h.assignments(), lists) and np.array_equal(h.codes(), codes)
    scanned = _check_search(oracle, h, cb, 0, Q, C_, lists, codes, 10, nlist, ctx="two rounds of slots")
    assert (scanned == n).all()
    h.set_profiling(True)
    _check_search(oracle, h, cb, 0, Q, C_, lists, codes, 200, nlist + 5, ctx="two rounds of slots, profiled, k 200")
    ms = h.last_timing()
    assert len(ms) == 5 and all(np.isfinite(t) and t >= 0 for t in ms) and ms[2] > 0 and ms[3] > 0, ms
    h.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_training_on_residuals(oracle):
    from longbow_amd import ivf, ivfpq, pq
    gpu_or_skip()
    X, Q = ro.clustered_case()
    nlist, M, k, nprobe = 16, 8, 10, 4
    cent, blob = ivfpq.train(X, nlist, M, residual=True)
    assert np.array_equal(cent, ivf.train(X, nlist))
    a = pqo.assign(oracle, 0, X, cent)
    want, _ = pq.train(ro.residuals(X, cent, a), M, 256)
    assert bytes(blob) == bytes(want)
    pcent, pblob = ivfpq.train(X, nlist, M, residual=False)
    assert np.array_equal(pcent, cent) and bytes(pblob) == bytes(pq.train(X, M, 256)[0])
    # recall@10 against the exact f32 k-NN of the probed rows
    truth = []
    for j in range(Q.shape[0]):
        rows = io.probed_rows(a, io.probes(oracle, 0, 0, Q[j], cent, nprobe))
        d = ((X[rows].astype(np.float64) - Q[j].astype(np.float64)) ** 2).sum(axis=1)
        truth.append(rows[np.argsort(d, kind="stable")[:k]])
        assert truth[-1].size == k
    recall = {}
    for residual, b in ((True, blob), (False, pblob)):
        h = ivfpq.IVFPQ(b, cent, residual=residual)
        h.add(X)
        assert np.array_equal(h.assignments(), a)
        lab, _ = h.search(Q, k, nprobe)
        recall[residual] = float(np.mean([np.intersect1d(lab[j], truth[j]).size / k for j in range(Q.shape[0])]))
        h.Close()
    print(f"recall@10: residual {recall[True]:.3f}, plain {recall[False]:.3f}")
    assert recall[True] > recall[False], recall


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_untouched_plain_path(oracle, parity):
    from longbow_amd import gpu
    X, Q, C_, cb, lists, codes = parity
    h, p = _handle(X, C_, cb), _handle(X, C_, cb, residual=False)
    # the centroids' copy is counted: codes three times, lists, assignments, the codebooks, the centroids twice
    n, M = X.shape[0], cb.shape[0]
    assert h.hbm_bytes >= n * (3 * M + 12) + cb.nbytes + 2 * C_.nbytes and p.hbm_bytes == h.hbm_bytes - C_.nbytes
    lib = h._lib
    kmax = LB_MAX_K + 1
    dist = np.full((Q.shape[0], kmax), 9.0, F)
    lab = np.full((Q.shape[0], kmax), 77, np.int64)
    args = (Q.shape[0], Q.ctypes.data)
    assert lib.lb_gpu_ivfpq_search(h._h, *args, kmax, 3, dist.ctypes.data, lab.ctypes.data) == UNSUPPORTED
    assert b"2048" in lib.lb_gpu_ivfpq_last_error(h._h)
    assert lib.lb_gpu_ivfpq_search(h._h, *args, 10, 0, dist.ctypes.data, lab.ctypes.data) == INVALID
    assert b"nprobe" in lib.lb_gpu_ivfpq_last_error(h._h)
    assert lib.lb_gpu_ivfpq_search(h._h, *args, 10, -4, dist.ctypes.data, lab.ctypes.data) == INVALID
    c = gpu.Cancel()
    c.fire()
    assert lib.lb_gpu_ivfpq_search_ctx(h._h, *args, 10, 3, dist.ctypes.data, lab.ctypes.data, c._h) == CANCELLED
    assert (dist == 9.0).all() and (lab == 77).all()
    _check_search(oracle, h, cb, 0, Q, C_, lists, codes, 10, 3, ctx="after the refusals")
    # a handle from lb_gpu_ivfpq_new is not residual and answers as the plain oracle says
    assert lib.lb_gpu_ivfpq_residual(p._h) == 0 and lib.lb_gpu_ivfpq_residual(h._h) == 1
    pcodes = pqo.encode(oracle, cb, X)
    assert np.array_equal(p.codes(), pcodes) and not np.array_equal(pcodes, codes)
    ol, od, _ = pqo.search(oracle, cb, 0, Q, C_, lists, pcodes, 10, 3)
    assert_same(*p.search(Q, 10, 3), ol, od, "the plain handle")
    p.Close()
    h.Close()
    e = _handle(X[:0], C_, cb)  # nothing stored: all padding
    el, ed = e.search(Q, 7, 2)
    assert (el == -1).all() and (ed == pqo.FLT_MAX).all() and e.last_search_stats() == (Q.shape[0], 0, 0, 0)
    e.Close()


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
