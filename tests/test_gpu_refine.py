"""lb_gpu_index_refine on the GPU against tests/refine_oracle.py (the refine semantics restated over the C oracle's batch_flat and
topk_canonical; tests/test_refine_semantics.py checks the restatement by hand): labels and distances must be equal, bit for bit.

The scan's geometry is ivf_scan_kernel's (128-row tiles, 64-element chunks; 256-row tiles in the generic form), so the shapes
are the ones around those edges: shortlists of 1, 2, 127, 128, 129, 1000 and 1025 entries, dimensions of one 16-byte piece, one
chunk, one chunk and a piece, a dimension only the generic form takes, and twelve chunks; 1, 3 and 70 queries; k of 1, 10, the
shortlist and beyond it.  One case has the largest shortlist (16,384) with the largest k, with enough queries that a workgroup
walks more than one tile."""
import threading

import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import ivfpq_oracle as pqo
from tests import refine_oracle as fo
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F, H = np.float32, np.float16
OK, INVALID, UNSUPPORTED, CANCELLED = 0, 1, 6, 8
LB_MAX_K, MAX_C = 2048, 16384
CS = (1, 2, 127, 128, 129, 1000, 1025)
NQS = (1, 3, 70)
KMODES = ("1", "10", "c", "c+5")


def new_index(dim, metric, f16=False, order=None):
    from longbow_amd import gpu
    gpu_or_skip()
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=dim, Metric=metric,
                                               DataType=gpu.DataType.Float16 if f16 else gpu.DataType.Float32))
    if order is not None:
        idx.set_order(order)
    return idx


def corpus(seed, n, dim, f16):
    """rows as the index takes them, and the f32 values the oracle reads"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(H if f16 else F)
    return X, X.astype(F)


def shortlists(rng, nq, c, n):
    """distinct rows in random order (c <= n)"""
    return np.stack([rng.permutation(n)[:c] for _ in range(nq)]).astype(np.int64)


def k_of(mode, c):
    return {"1": 1, "10": 10, "c": c, "c+5": c + 5}[mode]


# 1 ---------------------------------------------------------------------------------------------------------------------------
# Every (element type, D) with every metric and order; the (c, nq, k) triples rotate through their axes so that every value of
# every axis occurs several times over the grid (3 triples per combination, 54 combinations) without the full product.
@pytest.mark.parametrize("f16,dim", [(False, 4), (False, 64), (False, 68), (False, 100), (False, 768),
                                     (True, 8), (True, 72), (True, 100), (True, 768)])
def test_parity_grid(f16, dim):
    n = 5000
    X, Xf = corpus(dim + 1000 * f16, n, dim, f16)
    rng = np.random.default_rng(dim * 7 + f16)
    Q = rng.standard_normal((max(NQS), dim)).astype(F)
    turn = dim + 3 * f16
    for metric in (0, 1, 2):
        idx = new_index(dim, metric, f16)
        try:
            idx.Add(None, X)
            for order in (0, 1):
                for _ in range(3):
                    c, nq, km = CS[turn % len(CS)], NQS[turn % len(NQS)], KMODES[(turn // 3) % len(KMODES)]
                    turn += 1
                    k = k_of(km, c)
                    rows = shortlists(rng, nq, c, n)
                    lab, dist = idx.Refine(Q[:nq], rows, k, order)
                    ol, od = fo.refine(oc, metric, Q[:nq], Xf, rows, k, order)
                    assert_same(lab, dist, ol, od, f"f16 {f16} dim {dim} metric {metric} order {order} c {c} nq {nq} k {k}")
        finally:
            idx.Close()


def test_the_grid_keeps_every_value_of_every_axis():
    """the rotation of test_parity_grid, replayed: every c, nq and k mode occurs with f32 and with fp16 rows"""
    for f16, dims in ((False, (4, 64, 68, 100, 768)), (True, (8, 72, 100, 768))):
        seen = set()
        for dim in dims:
            turn = dim + 3 * f16
            for _ in range(18):
                seen |= {("c", CS[turn % len(CS)]), ("nq", NQS[turn % len(NQS)]), ("k", KMODES[(turn // 3) % len(KMODES)])}
                turn += 1
        assert seen == {("c", c) for c in CS} | {("nq", q) for q in NQS} | {("k", m) for m in KMODES}, (f16, seen)


def test_order_none_is_the_index_order():
    X, Xf = corpus(5, 3000, 64, False)
    rng = np.random.default_rng(6)
    Q = rng.standard_normal((5, 64)).astype(F)
    rows = shortlists(rng, 5, 300, 3000)
    for order in (0, 1):
        idx = new_index(64, 1, order=order)
        try:
            idx.Add(None, X)
            lab, dist = idx.Refine(Q, rows, 10)
            assert_same(lab, dist, *fo.refine(oc, 1, Q, Xf, rows, 10, order), f"order {order}")
        finally:
            idx.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16,dim,nq", [(False, 64, 40), (True, 64, 40), (False, 100, 70)])
def test_the_largest_shortlist_and_k(f16, dim, nq):
    """c = 16,384 = LB_REFINE_MAX_C, k = 2,048: 128 staged tiles over 103 workgroups a query at 40 queries, 64 generic tiles over
    59 at 70 queries, so some workgroups walk a second tile; the selection takes its radix path from the full LDS copy"""
    n, c, k = 20000, MAX_C, LB_MAX_K
    X, Xf = corpus(77 + dim, n, dim, f16)
    rng = np.random.default_rng(78)
    Q = rng.standard_normal((nq, dim)).astype(F)
    rows = shortlists(rng, nq, c, n)
    idx = new_index(dim, 0, f16)
    try:
        idx.Add(None, X)
        lab, dist = idx.Refine(Q, rows, k, 1)
        assert_same(lab, dist, *fo.refine(oc, 0, Q, Xf, rows, k, 1))
    finally:
        idx.Close()


@pytest.mark.parametrize("metric,order", [(0, 0), (1, 1)])
@pytest.mark.parametrize("f16", [False, True])
def test_one_workgroup_walks_several_tiles_and_chunks(f16, metric, order):
    """1,024 queries (one batch) with shortlists of 1,100 distinct rows: nine 128-row tiles, the last one partial, over four
    workgroups a query, so the first of them walks tiles 0, 4 and 8, in three chunks each (136 dims: 64 + 64 + 8), and the
    pipeline wraps from a tile's last chunk to the next tile's first"""
    TILE, CHUNK, GRID = 128, 64, 4096
    n, dim, nq, c, k = 3000, 136, 1024, 1100, 10
    tiles = -(-c // TILE)
    gx = min(tiles, max(1, -(-GRID // nq)))
    assert tiles >= 2 * gx + 1 and c % TILE != 0, (tiles, gx)
    assert -(-dim // CHUNK) >= 2 and dim % CHUNK != 0
    X, Xf = corpus(136 + f16, n, dim, f16)
    rng = np.random.default_rng(137)
    Q = rng.standard_normal((nq, dim)).astype(F)
    rows = shortlists(rng, nq, c, n)
    idx = new_index(dim, metric, f16)
    try:
        idx.Add(None, X)
        lab, dist = idx.Refine(Q, rows, k, order)
        assert_same(lab, dist, *fo.refine(oc, metric, Q, Xf, rows, k, order), f"f16 {f16} metric {metric} order {order}")
    finally:
        idx.Close()


def test_more_queries_than_a_batch_and_than_a_host_piece():
    """1,030 queries go in two device batches of at most 1,024; 600 shortlists of 16,384 entries go in two host pieces"""
    n, dim = 20000, 4
    X, Xf = corpus(9, n, dim, False)
    rng = np.random.default_rng(10)
    idx = new_index(dim, 0)
    try:
        idx.Add(None, X)
        Q = rng.standard_normal((1030, dim)).astype(F)
        rows = rng.integers(-2, n + 2, (1030, 8)).astype(np.int64)
        lab, dist = idx.Refine(Q, rows, 5, 0)
        assert_same(lab, dist, *fo.refine(oc, 0, Q, Xf, rows, 5, 0), "1030 queries")
        rows = rng.integers(0, n, (600, MAX_C)).astype(np.int64)  # (with repeats: about 11,000 distinct rows each)
        lab, dist = idx.Refine(Q[:600], rows, 5, 0)
        assert_same(lab, dist, *fo.refine(oc, 0, Q[:600], Xf, rows, 5, 0), "600 x 16384")
    finally:
        idx.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True])
def test_input_hygiene(f16):
    n, dim, k = 5000, 72, 20
    X, Xf = corpus(21, n, dim, f16)
    X[4001] = X[17]  # two identical vectors at different positions
    Xf[4001] = Xf[17]
    rng = np.random.default_rng(22)
    Q = rng.standard_normal((4, dim)).astype(F)
    Q[3] = Xf[17]
    good = shortlists(rng, 4, 200, n)
    good[3, :2] = (4001, 17)
    junk = np.array([-1, n, 2 ** 40, -(2 ** 62), n + 1, -2, 2 ** 31, 2 ** 32 + 5], np.int64)
    dirty = np.empty((4, 200 * 2 + 2 * junk.size + 3), np.int64)
    for j in range(4):
        parts = np.concatenate([good[j], good[j][::-1], junk, junk, good[j][:3]])  # every row twice or three times, junk between
        dirty[j] = parts[rng.permutation(parts.size)]
    dirty[2] = np.resize(junk, dirty.shape[1])  # a query whose list is all invalid
    idx = new_index(dim, 0, f16)
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    with_ids = new_index(dim, 0, f16)
    empty = new_index(dim, 0, f16)
    try:
        idx.Add(None, X)
        with_ids.Add(ids, X)
        lab, dist = idx.Refine(Q, dirty, k, 0)
        assert_same(lab, dist, *fo.refine(oc, 0, Q, Xf, dirty, k, 0), "dirty lists")
        cl, cd = idx.Refine(Q[[0, 1, 3]], np.sort(good[[0, 1, 3]], axis=1), k, 0)  # the cleaned ascending lists
        assert_same(lab[[0, 1, 3]], dist[[0, 1, 3]], cl, cd, "dirty against clean")
        assert (lab[2] == -1).all() and (dist[2] == fo.FLT_MAX).all()
        assert lab[3, :2].tolist() == [17, 4001] and dist[3, 0] == dist[3, 1] == 0.0  # a tie goes by row
        il, idist = with_ids.Refine(Q, dirty, k, 0)
        assert_same(il, idist, *fo.refine(oc, 0, Q, Xf, dirty, k, 0, ids=ids), "ids")
        assert np.array_equal(il, np.where(lab >= 0, lab * 3 + 11, -1))
        el, ed = empty.Refine(Q, dirty, k, 0)
        assert (el == -1).all() and (ed == fo.FLT_MAX).all()
    finally:
        idx.Close()
        with_ids.Close()
        empty.Close()


def test_the_row_filter_of_the_index_is_ignored():
    n, dim = 2000, 16
    X, Xf = corpus(31, n, dim, False)
    rng = np.random.default_rng(32)
    Q = rng.standard_normal((3, dim)).astype(F)
    rows = shortlists(rng, 3, 129, n)
    idx = new_index(dim, 0)
    try:
        idx.Add(None, X)
        idx.set_filter((np.arange(n) % 2).astype(np.uint8))
        lab, dist = idx.Refine(Q, rows, 10, 0)
        assert_same(lab, dist, *fo.refine(oc, 0, Q, Xf, rows, 10, 0))
        assert (lab % 2 == 0).any()
    finally:
        idx.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_whole_corpus_shortlist_is_the_search(metric):
    """a permutation of all rows as every query's shortlist: Refine is SearchBatch, bit for bit; on the float16 index with
    queries that are exact in fp16, against search_f16 of the same values"""
    n, dim, k = 3000, 64, 25
    rng = np.random.default_rng(40 + metric)
    Qh = rng.standard_normal((6, dim)).astype(H)
    rows = shortlists(rng, 6, n, n)
    for f16 in (False, True):
        X, _ = corpus(41, n, dim, f16)
        for order in (0, 1):
            idx = new_index(dim, metric, f16, order)
            try:
                idx.Add(None, X)
                sl, sd = idx.SearchBatch(Qh if f16 else Qh.astype(F), k)
                lab, dist = idx.Refine(Qh.astype(F), rows, k)
                assert_same(lab, dist, sl, sd, f"metric {metric} f16 {f16} order {order}")
            finally:
                idx.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def code_case():
    """3,000 x 32 clustered rows with their IVF partition (tests/ivfpq_oracle.py's 16-byte-form case) and an f32 index of them
    in order 0"""
    X, Q, C_, cb = pqo.parity_case(32, 16)
    idx = new_index(32, 0, order=0)
    idx.Add(None, X)
    yield X, Q, C_, cb, idx
    idx.Close()


def _handles(X, C_, cb):
    from longbow_amd import bq, ivfpq, pq, sq8
    b = bq.BQEncoder(32)
    b.add_vectors(X)
    s = sq8.train(X)
    s.add_vectors(X)
    p = pq.PQEncoder(pqo.blob(cb))
    p.add_codes(p.Encode(X))
    plain = ivfpq.IVFPQ(pqo.blob(cb), C_, 0)
    plain.add(X)
    resid = ivfpq.IVFPQ(pqo.blob(cb), C_, 0, residual=True)
    resid.add(X)
    search = {"bq": lambda q, c: b.search(q, c), "sq8": lambda q, c: s.search(q, c), "pq": lambda q, c: p.Search(q, c),
              "ivfpq": lambda q, c: plain.search(q, c, 3), "ivfpq residual": lambda q, c: resid.search(q, c, 3)}
    refine = {"bq": lambda i, q, k, c: b.search_refine(i, q, k, c), "sq8": lambda i, q, k, c: s.search_refine(i, q, k, c),
              "pq": lambda i, q, k, c: p.search_refine(i, q, k, c), "ivfpq": lambda i, q, k, c: plain.search_refine(i, q, k, c, 3),
              "ivfpq residual": lambda i, q, k, c: resid.search_refine(i, q, k, c, 3)}
    return {"bq": b, "sq8": s, "pq": p, "ivfpq": plain, "ivfpq residual": resid}, search, refine


def test_search_refine_is_the_handle_search_then_the_refine_oracle(code_case):
    X, Q, C_, cb, idx = code_case
    handles, search, refine = _handles(X, C_, cb)
    k, c = 10, 100
    mask = (np.arange(X.shape[0]) % 3 != 0).astype(np.uint8)
    try:
        for name, h in handles.items():
            short, _ = search[name](Q, c)
            assert (short >= 0).any()
            lab, dist = refine[name](idx, Q, k, c)
            assert_same(lab, dist, *fo.refine(oc, 0, Q, X, short, k, 0), name)
            h.set_filter(mask)  # a row filter on the code handle: visible rows only
            short, _ = search[name](Q, c)
            lab, dist = refine[name](idx, Q, k, c)
            assert_same(lab, dist, *fo.refine(oc, 0, Q, X, short, k, 0), name + " filtered")
            assert (mask[lab[lab >= 0]] == 1).all() and (lab >= 0).any(), name
    finally:
        for h in handles.values():
            h.Close()


def test_search_refine_on_a_float16_index_and_with_ids(code_case):
    from longbow_amd import ivfpq
    X, Q, C_, cb, _ = code_case
    Xh = X.astype(H)
    idx = new_index(32, 0, f16=True, order=0)
    h = ivfpq.IVFPQ(pqo.blob(cb), C_, 0, residual=True)
    with_ids = ivfpq.IVFPQ(pqo.blob(cb), C_, 0)
    try:
        idx.Add(None, Xh)
        h.add(X)
        short, _ = h.search(Q, 64, 2)
        lab, dist = h.search_refine(idx, Q, 5, 64, 2)
        assert_same(lab, dist, *fo.refine(oc, 0, Q, Xh.astype(F), short, 5, 0))
        with_ids.add(X, np.arange(X.shape[0], dtype=np.int64) + 10 ** 6)
        with pytest.raises(ValueError):
            with_ids.search_refine(idx, Q, 5, 64, 2)
    finally:
        idx.Close()
        h.Close()
        with_ids.Close()


def test_chained_on_a_stream(code_case):
    """IVF-PQ search_device into device labels, refine_device on the same stream: the host-pointer path's result"""
    import torch
    from longbow_amd import ivfpq
    X, Q, C_, cb, idx = code_case
    nq, c, k = Q.shape[0], 129, 10
    h = ivfpq.IVFPQ(pqo.blob(cb), C_, 0, residual=True)
    try:
        h.add(X)
        short, _ = h.search(Q, c, 4)
        want = idx.Refine(Q, short, k, 1)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            dq = torch.from_numpy(Q).cuda()
            d_short = torch.empty((nq, c), dtype=torch.int64, device="cuda")
            d_sdist = torch.empty((nq, c), dtype=torch.float32, device="cuda")
            d_lab = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            d_dist = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            stream.synchronize()
            h.search_device(nq, dq.data_ptr(), c, 4, d_sdist.data_ptr(), d_short.data_ptr(), stream=stream.cuda_stream)
            idx.refine_device(nq, dq.data_ptr(), c, d_short.data_ptr(), k, d_dist.data_ptr(), d_lab.data_ptr(), order=1,
                              stream=stream.cuda_stream)
        assert np.array_equal(d_short.cpu().numpy(), short)
        assert_same(d_lab.cpu().numpy(), d_dist.cpu().numpy(), *want)
        # and with no stream given: a private one
        d_lab.fill_(-7)
        torch.cuda.synchronize()
        idx.refine_device(nq, dq.data_ptr(), c, d_short.data_ptr(), k, d_dist.data_ptr(), d_lab.data_ptr(), order=1)
        assert_same(d_lab.cpu().numpy(), d_dist.cpu().numpy(), *want)
    finally:
        h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
PROPERTY_SEED = 0
PROPERTY_DRAWS = 48
PROPERTY_NQ = 6  # of the 48 draws of seed 0


def property_case(seed=PROPERTY_SEED):
    """4,000 x 32 rows around 16 centres, and of PROPERTY_DRAWS seeded queries near centres those whose distances over the rows
    are tie-free.  A query's 4,000 L2 distances lie within two or three binades of f32, so about one query in seven has none
    equal (measured on the CPU over 12,000 draws: 0.146): the draws of this seed leave PROPERTY_NQ queries, which the test
    asserts first, together with their being tie-free."""
    rng = np.random.default_rng(seed)
    centres = (rng.standard_normal((16, 32)) * 4).astype(F)
    X = (centres[rng.integers(0, 16, 4000)] + rng.standard_normal((4000, 32))).astype(F)
    Q = (centres[rng.integers(0, 16, PROPERTY_DRAWS)] + rng.standard_normal((PROPERTY_DRAWS, 32))).astype(F)
    return X, Q[[tie_free(X, q[None]) for q in Q]]


def tie_free(X, Q):
    return all(np.unique(oc.batch_flat(0, q, X, 0)).size == X.shape[0] for q in Q)


def test_refine_keeps_every_true_neighbour_the_shortlist_holds():
    """|refined & N10| == |shortlist & N10| per query, N10 the exact ten nearest: the refine loses nothing the shortlist had
    (exact distances without ties), and it is never below what the unrefined ADC top ten holds, which is part of the shortlist"""
    from longbow_amd import ivfpq
    gpu_or_skip()
    X, Q = property_case()
    assert Q.shape[0] == PROPERTY_NQ and tie_free(X, Q)
    N10, _ = oc.search_batch(0, Q, X, 10, order=0, nthreads=4)
    centroids, blob = ivfpq.train(X, 16, 8, residual=True)
    h = ivfpq.IVFPQ(blob, centroids, 0, residual=True)
    idx = new_index(32, 0, order=0)
    try:
        h.add(X)
        idx.Add(None, X)
        short, _ = h.search(Q, 100, 4)
        top, _ = h.search(Q, 10, 4)
        lab, _ = h.search_refine(idx, Q, 10, 100, 4)
        for j in range(Q.shape[0]):
            truth = set(N10[j].tolist())
            in_short = len(truth & set(short[j].tolist()))
            refined = len(truth & set(lab[j].tolist()))
            unrefined = len(truth & set(top[j].tolist()))
            assert set(top[j][top[j] >= 0].tolist()) <= set(short[j].tolist())
            assert refined == in_short, (j, refined, in_short)
            assert refined >= unrefined, (j, refined, unrefined)
    finally:
        h.Close()
        idx.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    X, Xf = corpus(50, 100, 16, False)
    idx = new_index(16, 0)
    idx.Add(None, X)
    yield idx, Xf
    idx.Close()


def _raw(lib, idx, nq, q, c, rows, k, order, dist, lab, device=False, ctx=None):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    if device:
        return lib.lb_gpu_index_refine_device_ctx(idx._h, nq, q, c, rows, k, order, dist, lab, None, ctx)
    return lib.lb_gpu_index_refine_ctx(idx._h, nq, p(q), c, p(rows), k, order, p(dist), p(lab), ctx)


def test_statuses(small):
    from longbow_amd import gpu
    lib = gpu_or_skip()
    idx, _ = small
    q = np.zeros((2, 16), F)
    rows = np.zeros((2, 4), np.int64)
    dist, lab = np.full((2, 3), 9.0, F), np.full((2, 3), 77, np.int64)
    assert _raw(lib, idx, 2, q, 4, rows, 3, -1, dist, lab) == OK
    dist[:], lab[:] = 9.0, 77
    for c in (0, -1, MAX_C + 1):
        assert _raw(lib, idx, 2, q, c, rows, 3, -1, dist, lab) == INVALID
    for k in (0, -1):
        assert _raw(lib, idx, 2, q, 4, rows, k, -1, dist, lab) == INVALID
    assert _raw(lib, idx, 2, q, 4, rows, LB_MAX_K + 1, -1, dist, lab) == UNSUPPORTED
    assert "exceeds the supported maximum" in lib.lb_gpu_last_error(idx._h).decode()
    assert _raw(lib, idx, -1, q, 4, rows, 3, -1, dist, lab) == INVALID
    for order in (-2, 2):
        assert _raw(lib, idx, 2, q, 4, rows, 3, order, dist, lab) == INVALID
    for args in ((None, rows, dist, lab), (q, None, dist, lab), (q, rows, None, lab), (q, rows, dist, None)):
        assert _raw(lib, idx, 2, args[0], 4, args[1], 3, -1, args[2], args[3]) == INVALID
    assert _raw(lib, idx, 0, None, 4, None, 3, -1, None, None) == OK  # nq == 0
    assert lib.lb_gpu_index_refine(idx._h, 0, None, 4, None, 3, -1, None, None) == OK
    assert lib.lb_gpu_index_refine_device_ctx(idx._h, 0, None, 4, None, 3, -1, None, None, None, None) == OK
    assert lib.lb_gpu_index_refine_device_ctx(idx._h, 2, None, 4, None, 3, -1, None, None, None, None) == INVALID
    fired = gpu.Cancel()
    try:
        fired.fire()
        assert _raw(lib, idx, 2, q, 4, rows, 3, -1, dist, lab, ctx=fired._h) == CANCELLED
        assert lib.lb_gpu_last_error(idx._h).decode() == "context canceled"
        with pytest.raises(gpu.Canceled):
            idx.Refine(q, rows, 3, ctx=fired)
    finally:
        fired.close()
    assert (dist == 9.0).all() and (lab == 77).all()  # a refused call writes nothing
    # k > c is allowed: padding
    l2, d2 = idx.Refine(q, rows, 3)
    assert (l2[:, 0] == 0).all() and (l2[:, 1:] == -1).all() and (d2[:, 1:] == fo.FLT_MAX).all()


def test_an_int8_index_is_refused_with_a_text():
    from longbow_amd import gpu
    lib = gpu_or_skip()
    i8 = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=16, Metric=0, DataType=gpu.DataType.Int8))
    try:
        i8.Add(None, np.ones((10, 16), np.int8))
        q, rows = np.zeros((1, 16), F), np.zeros((1, 2), np.int64)
        dist, lab = np.zeros((1, 1), F), np.zeros((1, 1), np.int64)
        assert _raw(lib, i8, 1, q, 2, rows, 1, -1, dist, lab) == UNSUPPORTED
        assert lib.lb_gpu_last_error(i8._h).decode() == "refine reads float32 or float16 rows: not available on an int8 index"
        with pytest.raises(gpu.LongbowGPUError):
            i8.Refine(q, rows, 1)
    finally:
        i8.Close()


def test_eight_threads_on_one_handle():
    n, dim, k = 5000, 64, 10
    X, Xf = corpus(60, n, dim, False)
    idx = new_index(dim, 0)
    rng = np.random.default_rng(61)
    work = [(rng.standard_normal((9, dim)).astype(F), shortlists(rng, 9, 300 + 17 * t, n)) for t in range(8)]
    want = [fo.refine(oc, 0, q, Xf, r, k, 1) for q, r in work]
    got = [None] * 8
    errs = []

    def run(t):
        try:
            for _ in range(3):
                got[t] = idx.Refine(work[t][0], work[t][1], k, 1)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    try:
        idx.Add(None, X)
        threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errs, errs
        for t in range(8):
            assert_same(got[t][0], got[t][1], *want[t], f"thread {t}")
    finally:
        idx.Close()
