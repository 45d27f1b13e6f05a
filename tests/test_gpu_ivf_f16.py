"""lb_gpu_ivf_new_f16 on the GPU: an IVF-Flat handle whose rows are float16 must be indistinguishable, bit for bit, from the
float32 handle over the widened rows.  So the oracle is the existing one (tests/ivf_oracle.py, tests/ivf_filter_cases.py) called
with X16.astype(float32), and where a case is too large for it the yardstick is a float32 IVFFlat over the widened rows in the
same test (oracle-tested in tests/test_gpu_ivf.py).  In every case "rows" means X.astype(float16) of the shared inputs.  The
shapes are the smallest at which the fp16 list scan can go wrong: dimensions of one 16-byte piece, a partial 128-element chunk,
exactly one, one plus a piece and six; dimensions that take the one-lane-per-row form; lists around the 128-row tile; a workgroup
that walks several tiles of several chunks; an add that crosses the 65,536-row assignment piece."""
import numpy as np
import pytest

from tests import ivf_filter_cases as fc
from tests import ivf_oracle as io
from tests import row_view_cases as rv
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F, H = np.float32, np.float16
INVALID = 1
LDS_KEYS = 16384  # IVF_SELECT_LDS_KEYS: a query with more scanned rows is selected from global memory


def _f16(X16, C_, metric=0, order=0, ids=None):
    from longbow_amd import ivf
    from longbow_amd.gpu import DataType
    gpu_or_skip()
    assert X16.dtype == H
    h = ivf.IVFFlat(C_, metric, order, dtype=DataType.Float16)
    if X16.shape[0]:
        h.add(X16, ids)
    return h


def _f32(X, C_, metric=0, order=0, ids=None):
    from longbow_amd import ivf
    gpu_or_skip()
    assert X.dtype == F
    h = ivf.IVFFlat(C_, metric, order)
    if X.shape[0]:
        h.add(X, ids)
    return h


def _check_search(oracle, h, metric, order, Q, W, C_, lists, k, nprobe, ids=None, ctx=""):
    """W: the widened rows"""
    ol, od, scanned = io.search(oracle, metric, order, Q, W, C_, lists, k, nprobe, ids=ids)
    lab, dist = h.search(Q, k, nprobe)
    assert_same(lab, dist, ol, od, ctx)
    st = h.last_search_stats()
    assert st[0] == Q.shape[0] and st[1] == int(scanned.sum()) and st[2] == int(scanned.max()), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= LDS_KEYS).sum()), (st, ctx)
    return scanned


def _same_handles(h16, h32, Q, k, nprobe, ctx=""):
    """labels, distances (NaN included), assignments, list sizes and stats of the two handles are equal"""
    assert h16.ntotal == h32.ntotal
    assert np.array_equal(h16.assignments(), h32.assignments()), ctx
    assert np.array_equal(h16.list_sizes(), h32.list_sizes()), ctx
    l16, d16 = h16.search(Q, k, nprobe)
    s16 = h16.last_search_stats()
    l32, d32 = h32.search(Q, k, nprobe)
    assert np.array_equal(l16, l32), f"labels differ {ctx}: {np.argwhere(l16 != l32)[:5]}"
    assert np.array_equal(d16, d32, equal_nan=True), f"distances differ {ctx}: {np.argwhere(~((d16 == d32) | (np.isnan(d16) & np.isnan(d32))))[:5]}"
    assert s16 == h32.last_search_stats(), ctx
    return l16, d16


@pytest.fixture(scope="module")
def parity(oracle):
    """the shape of case 1 as fp16 rows, with the oracle's lists of the widened rows at metric 0, order 0"""
    X, Q, C_ = io.parity_case()
    X16 = X.astype(H)
    W = X16.astype(F)
    return X16, W, Q, C_, io.assign(oracle, 0, 0, W, C_)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_parity_grid(oracle, parity, metric, order):
    X16, W, Q, C_, lists0 = parity
    lists = lists0 if (metric, order) == (0, 0) else io.assign(oracle, metric, order, W, C_)
    h = _f16(X16, C_, metric, order)
    assert h.dtype == 1 and h.ntotal == X16.shape[0] and (h.nlist, h.dims) == C_.shape
    assert np.array_equal(h.assignments(), lists)
    assert np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    assert np.array_equal(h.centroids(), C_)
    for nprobe in (1, 3, 16):
        _check_search(oracle, h, metric, order, Q, W, C_, lists, 10, nprobe, ctx=f"metric {metric} order {order} nprobe {nprobe}")
    h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_two_identities(parity, metric):
    """the float32 handle over the widened rows (queries that are not fp16-representable), and with every list probed and fp16
    queries the float16 flat index over the same rows"""
    from longbow_amd import gpu
    X16, W, Q, C_, _ = parity
    assert not np.array_equal(Q.astype(H).astype(F), Q)
    Q16 = Q.astype(H)
    for order in (0, 1):
        h16, h32 = _f16(X16, C_, metric, order), _f32(W, C_, metric, order)
        assert (h16.dtype, h32.dtype) == (1, 0)
        for nprobe in (1, 3, 16):
            _same_handles(h16, h32, Q, 10, nprobe, f"metric {metric} order {order} nprobe {nprobe}")
        flat = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=X16.shape[1], Metric=metric, DataType=gpu.DataType.Float16))
        flat.set_order(order)
        flat.Add(None, X16)
        fl, fd = flat.SearchBatch(Q16, 10)
        for nprobe in (16, 21):
            for queries in (Q16, Q16.astype(F)):  # float16 queries are widened on the host
                lab, dist = h16.search(queries, 10, nprobe)
                assert_same(lab, dist, fl, fd, f"flat fp16, metric {metric} order {order} nprobe {nprobe}")
            assert h16.last_search_stats()[1] == Q.shape[0] * X16.shape[0]
        for x in (flat, h16, h32):
            x.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3, 4, 5, 12, 100, 8, 16, 120, 128, 136, 768])
def test_dimensions(oracle, dim):
    """1, 3, 4, 5, 12, 100: the one-lane-per-row form (D % 8 != 0); 8: one piece; 16, 120: a partial chunk; 128: exactly one chunk;
    136: one chunk plus one piece; 768: six chunks"""
    n, nlist, nprobe, k, nq = (3000, 16, 4, 100, 3) if dim == 768 else (1000, 7, 2, 10, 9)
    X, Q, C_ = io.parity_case(n, dim, nlist, nq, seed=dim)
    X16 = X.astype(H)
    W = X16.astype(F)
    for metric, order in ((0, 0), (1, 1), (2, 1), (0, 1)):
        lists = io.assign(oracle, metric, order, W, C_)
        h = _f16(X16, C_, metric, order)
        assert np.array_equal(h.assignments(), lists)
        _check_search(oracle, h, metric, order, Q, W, C_, lists, k, nprobe, ctx=f"dim {dim} metric {metric} order {order}")
        h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_list_length_edges(oracle):
    counts = (0, 1, 127, 128, 129, 257)
    X, Q, C_, owner = io.edge_case(counts)
    X16 = X.astype(H)  # (at 100 the fp16 grid is 1/16: many rows of a list are equal, and the row number breaks the ties)
    W = X16.astype(F)
    h = _f16(X16, C_)
    assert np.array_equal(h.assignments(), owner) and h.list_sizes().tolist() == list(counts)
    for nprobe in (1, 2):
        for k in (10, 200):
            _check_search(oracle, h, 0, 0, Q, W, C_, owner, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
    lab, dist = h.search(Q, 10, 1)
    assert (lab[0] == -1).all() and (dist[0] == io.FLT_MAX).all()  # an empty probed list: all padding
    assert lab[1, 0] == np.flatnonzero(owner == 1)[0] and (lab[1, 1:] == -1).all() and (dist[1, 1:] == io.FLT_MAX).all()
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_one_workgroup_walks_several_tiles_and_chunks():
    """1024 queries x 4 probes = 4,096 pairs, so the scan's grid has one workgroup per (query, list): it walks the three tiles of a
    list of about 300 rows, two chunks each (136 dims), and the pipeline wraps from a tile's last chunk to the next tile's first"""
    X, Q, C_ = io.parity_case(2400, 136, 8, 1024, seed=136)
    X16 = X.astype(H)
    h16, h32 = _f16(X16, C_), _f32(X16.astype(F), C_)
    sizes = h16.list_sizes()
    assert sizes.max() > 256, sizes  # (three tiles at least)
    _same_handles(h16, h32, Q, 10, 4, "several tiles and chunks")
    h16.Close()
    h32.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_skew_and_the_long_selection(oracle):
    X, Q, C_ = io.skew_case()
    X16 = X.astype(H)
    W = X16.astype(F)
    lists = io.assign(oracle, 0, 0, W, C_)
    h = _f16(X16, C_)
    assert np.array_equal(h.assignments(), lists)
    for nprobe in (1, 2):
        for k in (1, 2048):
            _check_search(oracle, h, 0, 0, Q, W, C_, lists, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
    h.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_adds_in_pieces_with_ids(oracle, parity):
    import torch
    from longbow_amd import ivf
    X16, W, Q, C_, lists = parity
    n = X16.shape[0]
    rng = np.random.default_rng(7)
    ids = rng.permutation(1 << 20)[:n].astype(np.int64) + (np.arange(n, dtype=np.int64) % 3 << 41)
    assert np.unique(ids).size == ids.size and (ids > 1 << 40).any()
    one = _f16(X16, C_, ids=ids)
    pieces = _f16(X16[:0], C_)
    dev = _f16(X16[:0], C_)
    dX, dI = torch.from_numpy(X16).cuda(), torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    r0 = 0
    for cnt in (127, 1000, 1873):
        pieces.add(X16[r0:r0 + cnt], ids[r0:r0 + cnt])
        dev.add_device(cnt, dX[r0:].data_ptr(), dI[r0:].data_ptr())
        r0 += cnt
        assert pieces.ntotal == r0 and dev.ntotal == r0
        assert np.array_equal(pieces.assignments(), lists[:r0]) and np.array_equal(dev.assignments(), lists[:r0])
        assert np.array_equal(pieces.list_sizes(), np.bincount(lists[:r0], minlength=C_.shape[0]))
        ol, od, _ = io.search(oracle, 0, 0, Q, W[:r0], C_, lists[:r0], 10, 3, ids=ids[:r0])
        assert_same(*pieces.search(Q, 10, 3), ol, od, f"host adds, {r0} rows")
        assert_same(*dev.search(Q, 10, 3), ol, od, f"device-pointer adds, {r0} rows")
    assert r0 == n
    assert_same(*one.search(Q, 10, 3), ol, od, "one add, ids")
    assert np.array_equal(dev.list_sizes(), one.list_sizes())
    # ids on every add or on none, as on a float32 handle
    for h, bad in ((pieces, None), (_f16(X16[:5], C_), ids[:3])):
        before = h.ntotal
        rc = h._lib.lb_gpu_ivf_add_f16(h._h, 3, X16.ctypes.data, bad.ctypes.data if bad is not None else None)
        assert rc == INVALID and h.ntotal == before
        with pytest.raises(ivf._lib.LongbowGPUError, match="ids"):
            h.add(X16[:3], bad)
        assert h.ntotal == before
    assert_same(*pieces.search(Q, 10, 3), ol, od, "after the refused add")
    for h in (one, pieces, dev):
        h.Close()


def test_an_add_that_crosses_the_assignment_piece():
    """65,536 + 129 rows in one add: the rows are widened and assigned in two pieces"""
    n = 65536 + 129
    X, Q, C_ = io.parity_case(n, 8, 4, 5, seed=65)
    X16 = X.astype(H)
    h16, h32 = _f16(X16, C_), _f32(X16.astype(F), C_)
    assert h16.ntotal == n
    _same_handles(h16, h32, Q, 10, 2, "65,665 rows")
    h16.Close()
    h32.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [8, 12])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_values(metric, dim):
    """+-inf, NaN, fp16 subnormals, +-65504 and +-0 in the rows, in the staged (dim 8) and the one-lane-per-row (dim 12) form:
    every row of the probed lists is reported (k = n), in the float32 handle's order, NaN last"""
    rng = np.random.default_rng(9)
    n, nlist = 700, 6
    X16 = rng.standard_normal((n, dim)).astype(H)
    C_ = X16[[3, 100, 200, 300, 400, 500]].astype(F)
    X16[17, 4] = np.nan
    X16[18, 0] = np.inf
    X16[19] = 0.0
    X16[20, 1] = -np.inf
    X16[21] = H(2.0 ** -24)  # the smallest fp16 subnormal
    X16[22] = H(2.0 ** -15)  # half the smallest normal
    X16[23, 2], X16[23, 3] = H(65504.0), H(-65504.0)
    X16[24] = -0.0
    X16[25, ::2] = H(-2.0 ** -24)
    W = X16.astype(F)
    assert W[21, 0] == F(2.0 ** -24) and W[22, 0] == F(2.0 ** -15) and np.signbit(W[24]).all()
    Q = rng.standard_normal((4, dim)).astype(F)
    Q[3, 2] = np.nan
    Q[2] *= F(1.0e4)  # (products with the subnormal rows that are normal f32 numbers)
    for order in (0, 1):
        h16, h32 = _f16(X16, C_, metric, order), _f32(W, C_, metric, order)
        _same_handles(h16, h32, Q, n, 3, f"metric {metric} order {order} dim {dim} nprobe 3")
        lab, _ = _same_handles(h16, h32, Q, n, nlist, f"metric {metric} order {order} dim {dim}, every list")
        assert (np.sort(lab, axis=1) == np.arange(n)).all()  # (every row is reported, the special ones too)
        h16.Close()
        h32.Close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_filters_at_the_tile_edges(oracle):
    X, Q, C_, owner = io.edge_case(fc.EDGE_COUNTS)
    X16 = X.astype(H)
    W = X16.astype(F)
    mask = fc.keep_per_list(owner, fc.EDGE_KEEP)
    h = _f16(X16, C_)
    h.set_filter(mask)
    assert h.nvisible() == sum(fc.EDGE_KEEP) and h.list_sizes().tolist() == list(fc.EDGE_COUNTS)
    for nprobe in (1, 2):
        ol, od, scanned = fc.search_filtered(oracle, 0, 0, Q, W, C_, owner, mask, fc.K, nprobe)
        assert_same(*h.search(Q, fc.K, nprobe), ol, od, f"nprobe {nprobe}")
        assert h.last_search_stats()[:3] == (Q.shape[0], int(scanned.sum()), int(scanned.max()))
        if nprobe == 1:
            assert scanned.tolist() == list(fc.EDGE_KEEP)
    h.Close()


def test_filter_column_an_add_under_a_filter_and_clearing(oracle, parity):
    X16, W, Q, C_, lists = parity
    n = X16.shape[0]
    rng = np.random.default_rng(17)
    col = rv.int64_edge_column(n)
    valid = rng.random(n) < 0.8

    def check(h, rows, mask, ctx):
        ol, od, scanned = fc.search_filtered(oracle, 0, 0, Q, W[:rows], C_, lists[:rows], mask, fc.K, 3)
        assert h.nvisible() == np.count_nonzero(mask), ctx
        assert_same(*h.search(Q, fc.K, 3), ol, od, ctx)
        assert h.last_search_stats()[:3] == (Q.shape[0], int(scanned.sum()), int(scanned.max())), ctx

    h = _f16(X16[:1000], C_)
    h.filter_column(col[:1000], 2 ** 32, rv.GE, valid=rv.validity_bitmap(valid[:1000], 3), validity_offset=3)
    m = rv.predicate(col[:1000], 2 ** 32, rv.GE, valid[:1000])
    assert 0 < np.count_nonzero(m) < 1000
    check(h, 1000, m, "filter_column, int64 with a validity bitmap")
    h.add(X16[1000:])  # the new rows are visible
    full = np.concatenate([m, np.ones(n - 1000, np.uint8)])
    assert h.ntotal == n and np.array_equal(h.assignments(), lists)
    check(h, n, full, "an add under a filter")
    h.reserve(20000)  # a change of capacity keeps the filter and the fp16 rows
    check(h, n, full, "after reserve")
    h.set_filter(None)
    assert h.nvisible() == n
    _check_search(oracle, h, 0, 0, Q, W, C_, lists, 10, 3, ctx="filter cleared")
    h.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_misaligned_queries(parity):
    """a query pointer 4 bytes off a 16-byte boundary takes the one-lane-per-row form: same answers"""
    import torch
    X16, W, Q, C_, _ = parity
    h = _f16(X16, C_, 1, 1)
    nq, dim = Q.shape
    buf = torch.zeros(nq * dim + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dQ = torch.from_numpy(Q).cuda()
    buf[1:1 + nq * dim] = dQ.reshape(-1)
    out = []
    for ptr in (dQ.data_ptr(), buf.data_ptr() + 4):
        dD = torch.full((nq, 10), -5.0, dtype=torch.float32, device="cuda")
        dL = torch.full((nq, 10), -5, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        h.search_device(nq, ptr, 10, 3, dD.data_ptr(), dL.data_ptr())
        out.append((dL.cpu().numpy(), dD.cpu().numpy()))
    assert dQ.data_ptr() % 16 == 0 and (buf.data_ptr() + 4) % 16 == 4
    assert_same(*out[1], *out[0], "misaligned queries")
    assert_same(*out[0], *h.search(Q, 10, 3), "device-pointer search")
    h.Close()


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_refusals_behind_a_live_handle(parity):
    import torch
    X16, W, Q, C_, _ = parity
    h16, h32 = _f16(X16[:500], C_), _f32(W[:500], C_)
    lib = h16._lib
    dW, dX = torch.from_numpy(W[:3].copy()).cuda(), torch.from_numpy(X16[:3].copy()).cuda()
    torch.cuda.synchronize()
    for n in (3, 0):
        assert lib.lb_gpu_ivf_add(h16._h, n, W.ctypes.data, None) == INVALID
        assert b"float16" in lib.lb_gpu_ivf_last_error(h16._h)
        assert lib.lb_gpu_ivf_add_device(h16._h, n, dW.data_ptr(), None) == INVALID
        assert lib.lb_gpu_ivf_add_f16(h32._h, n, X16.ctypes.data, None) == INVALID
        assert b"float32" in lib.lb_gpu_ivf_last_error(h32._h)
        assert lib.lb_gpu_ivf_add_f16_device(h32._h, n, dX.data_ptr(), None) == INVALID
    assert h16.ntotal == 500 and h32.ntotal == 500
    with pytest.raises(TypeError):
        h16.add(W[:3])  # (float32 data is not converted silently)
    assert h16.ntotal == 500
    _same_handles(h16, h32, Q, 10, 3, "after the refused adds")
    h16.Close()
    h32.Close()


# 12 --------------------------------------------------------------------------------------------------------------------------
def test_bytes():
    C_ = np.eye(4, 16, dtype=F)
    h16, h32 = _f16(np.empty((0, 16), H), C_), _f32(np.empty((0, 16), F), C_)
    assert h16.hbm_bytes == h32.hbm_bytes
    h16.reserve(5000)
    h32.reserve(5000)
    assert h32.hbm_bytes - h16.hbm_bytes == 5000 * 16 * 2
    h16.Close()
    h32.Close()


# 13 --------------------------------------------------------------------------------------------------------------------------
def test_python_mirror(parity):
    from longbow_amd import ivf
    from longbow_amd.gpu import DataType
    X16, W, Q, C_, lists = parity
    n = X16.shape[0]
    ids = np.arange(n, dtype=np.int64) * 7 + (1 << 33)
    h = _f16(X16, C_)
    lab, dist = h.search(Q, 10, 3)
    want = np.where(lab >= 0, ids[np.clip(lab, 0, None)], -1)
    idx = ivf.IVFFlatIndex(16, ivf.IVFFlatConfig(NClusters=16, NProbe=3), centroids=C_, data_type=DataType.Float16)
    idx.AddBatch(ids[:2000], X16[:2000])
    idx.Add(ids[2000], X16[2000])
    assert idx.Size() == 2001
    with pytest.raises(TypeError):
        idx.AddBatch(ids[:2], W[:2])
    idx.Build()
    idx.AddBatch(ids[2001:], X16[2001:])  # after Build(): straight to the handle
    assert idx.Size() == n and idx._h.dtype == 1
    assert_same(*idx.SearchBatch(Q, 10), want, dist, "SearchBatch")
    assert np.array_equal(idx.assignments(), lists) and np.array_equal(idx.list_sizes(), h.list_sizes())
    idx.Close()
    # Build() without centroids trains them on the widened rows: every list probed is the exhaustive answer
    t = ivf.IVFFlatIndex(16, ivf.IVFFlatConfig(NClusters=8, NProbe=8), train_iters=2, data_type=DataType.Float16)
    t.AddBatch(np.arange(500), X16[:500])
    t.Build()
    full = _f16(X16[:500], C_)
    assert_same(*t.SearchBatch(Q, 5), *full.search(Q, 5, 16), "trained, every list probed")
    for x in (t, full, h):
        x.Close()
