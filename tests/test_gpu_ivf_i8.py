"""lb_gpu_ivf_new_i8 on the GPU: an IVF-Flat handle over int8 rows, searched with int8 queries.  The oracle is
tests/ivf_i8_oracle.py: lists and probes from tests/ivf_oracle.py over the widened rows and queries, distances from
tests/i8_oracle.py (the reference's DataTypeInt8 kernels).  "Rows" are int8 throughout; where a case starts from a float case of
ivf_oracle it is scaled and rounded into int8 here.  The shapes are the smallest at which the int8 list scan can go wrong:
dimensions of one 16-byte piece, a partial 256-byte stage, exactly one, one plus a piece, several, the last staged one of dot,
and dimensions that take the one-lane-per-row form; lists around the 128-row tile; a workgroup that walks several tiles of several
stages; values at the ends of the int32 sums; an add that crosses the 65,536-row assignment piece."""
import numpy as np
import pytest

from tests import i8_oracle as i8
from tests import ivf_filter_cases as fc
from tests import ivf_i8_oracle as o8
from tests import ivf_oracle as io
from tests import row_view_cases as rv
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F, B = np.float32, np.int8
INVALID, UNSUPPORTED, CANCELLED = 1, 6, 8
LB_MAX_K = 2048
LDS_KEYS = 16384  # IVF_SELECT_LDS_KEYS: a query with more scanned rows is selected from global memory
TILE = 128        # rows per tile of the staged scan


def _i8(X8, C_, metric=0, order=0, ids=None):
    from longbow_amd import ivf
    gpu_or_skip()
    assert X8.dtype == B
    h = ivf.IVFFlatInt8(C_, metric, order)
    if X8.shape[0]:
        h.add(X8, ids)
    return h


def _f32(X, C_, metric=0, order=0):
    from longbow_amd import ivf
    gpu_or_skip()
    assert X.dtype == F
    h = ivf.IVFFlat(C_, metric, order)
    if X.shape[0]:
        h.add(X)
    return h


def _flat_i8(X8, metric, order=0):
    from longbow_amd import gpu
    gpu_or_skip()
    flat = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=X8.shape[1], Metric=metric, DataType=gpu.DataType.Int8))
    flat.set_order(order)
    flat.Add(None, X8)
    return flat


def _check_search(oracle, h, metric, order, Q8, X8, C_, lists, k, nprobe, ids=None, mask=None, ctx=""):
    ol, od, scanned = o8.search(oracle, metric, order, Q8, X8, C_, lists, k, nprobe, ids=ids, mask=mask)
    lab, dist = h.search(Q8, k, nprobe)
    assert_same(lab, dist, ol, od, ctx)
    st = h.last_search_stats()
    assert st[0] == Q8.shape[0] and st[1] == int(scanned.sum()) and st[2] == int(scanned.max()), (st, scanned.sum(), scanned.max(), ctx)
    assert st[3] == int((scanned <= LDS_KEYS).sum()), (st, ctx)
    return scanned


def _random_case(n, dim, nlist, nq, seed):
    """full-range int8 rows and queries; the centroids are nlist of the rows, widened"""
    rng = np.random.default_rng(seed)
    X8 = rng.integers(-128, 128, (n, dim)).astype(B)
    Q8 = rng.integers(-128, 128, (nq, dim)).astype(B)
    C_ = X8[np.sort(rng.permutation(n)[:nlist])].astype(F)
    return X8, Q8, C_


@pytest.fixture(scope="module")
def parity(oracle):
    """the shape of ivf_oracle.parity_case() as int8 rows and queries (30 to a standard deviation), with the oracle's lists at
    metric 0, order 0"""
    X, Q, C_ = io.parity_case()
    X8, Q8, C_ = o8.to_i8(X, 30), o8.to_i8(Q, 30), (C_ * F(30)).astype(F)
    assert X8.min() < -100 and X8.max() > 100
    return X8, Q8, C_, o8.assign(oracle, 0, 0, X8, C_)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("metric", [0, 2])
def test_parity_grid(oracle, parity, metric, order):
    X8, Q8, C_, lists0 = parity
    lists = lists0 if (metric, order) == (0, 0) else o8.assign(oracle, metric, order, X8, C_)
    h = _i8(X8, C_, metric, order)
    assert h.dtype == 2 and h.ntotal == X8.shape[0] and (h.nlist, h.dims) == C_.shape
    assert np.array_equal(h.assignments(), lists)
    assert np.array_equal(h.list_sizes(), np.bincount(lists, minlength=C_.shape[0]))
    assert np.array_equal(h.centroids(), C_)
    for nprobe in (1, 3, 16):
        _check_search(oracle, h, metric, order, Q8, X8, C_, lists, 10, nprobe, ctx=f"metric {metric} order {order} nprobe {nprobe}")
    h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2])
def test_two_identities(parity, metric):
    """with every list probed the flat int8 index over the same rows; assignments and list sizes of a float32 handle over the
    widened rows"""
    X8, Q8, C_, _ = parity
    flat = _flat_i8(X8, metric)
    fl, fd = flat.SearchBatch(Q8, 10)
    for order in (0, 1):
        h8, h32 = _i8(X8, C_, metric, order), _f32(X8.astype(F), C_, metric, order)
        assert (h8.dtype, h32.dtype) == (2, 0)
        assert np.array_equal(h8.assignments(), h32.assignments()), (metric, order)
        assert np.array_equal(h8.list_sizes(), h32.list_sizes()), (metric, order)
        for nprobe in (16, 21):
            lab, dist = h8.search(Q8, 10, nprobe)
            assert_same(lab, dist, fl, fd, f"flat int8, metric {metric} order {order} nprobe {nprobe}")
            assert np.array_equal(np.signbit(dist), np.signbit(fd))
            assert h8.last_search_stats()[1] == Q8.shape[0] * X8.shape[0]
        h8.Close()
        h32.Close()
    flat.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [16, 48, 256, 272, 528, 1024, 1040, 2048, 8, 20, 100])
def test_dimensions(oracle, dim):
    """16: one piece; 48: a partial stage; 256: exactly one stage; 272: a stage and a piece; 528: two stages and a piece; 1024:
    dot's last staged dimension; 1040, 2048: L2 staged, dot one lane per row; 8, 20, 100: one lane per row, L2 with 8, 4 and 4
    tail elements behind 0, 1 and 6 blocks of 16"""
    X8, Q8, C_ = _random_case(600, dim, 4, 5, seed=dim)
    for metric, order in ((0, 0), (2, 1)):
        lists = o8.assign(oracle, metric, order, X8, C_)
        h = _i8(X8, C_, metric, order)
        assert np.array_equal(h.assignments(), lists)
        for nprobe in (2, 4):
            _check_search(oracle, h, metric, order, Q8, X8, C_, lists, 10, nprobe, ctx=f"dim {dim} metric {metric} nprobe {nprobe}")
        h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_values_l2_2048_is_not_the_f32_chain(oracle):
    """rows and queries uniform over -128..127 at D = 2048: the reference's f32 chain over the widened values rounds where the
    int8 kernel's int32 sum does not, so a scan that merely widens cannot pass"""
    rng = np.random.default_rng(7)
    X8 = rng.integers(-128, 128, (64, 2048)).astype(B)
    Q8 = rng.integers(-128, 128, (4, 2048)).astype(B)
    want = i8.l2_values(Q8, X8)
    W = X8.astype(F)
    chain = np.stack([np.asarray(oracle.batch_flat(0, Q8[j].astype(F), W, 0), F) for j in range(4)])
    assert (chain.view(np.uint32) != want.view(np.uint32)).any()
    C_ = X8[[5, 40]].astype(F)
    lists = o8.assign(oracle, 0, 0, X8, C_)
    h = _i8(X8, C_)
    for nprobe in (1, 2):
        _check_search(oracle, h, 0, 0, Q8, X8, C_, lists, 64, nprobe, ctx=f"uniform, D 2048, nprobe {nprobe}")
    h.Close()


def test_values_at_the_ends_of_the_sums(oracle):
    # L2 at D = 8192, rows of -128 against a query of 127: the largest sum, 8192 * 255^2 = 532,684,800
    rng = np.random.default_rng(11)
    X8 = rng.integers(-128, 128, (TILE + 3, 8192)).astype(B)
    X8[::7] = -128
    Q8 = np.full((2, 8192), 127, B)
    Q8[1] = rng.integers(-128, 128, 8192)
    C_ = np.stack([np.full(8192, -100.0, F), np.zeros(8192, F)])
    lists = o8.assign(oracle, 0, 0, X8, C_)
    assert set(lists[::7]) == {0}
    h = _i8(X8, C_)
    lab, dist = h.search(Q8, 200, 2)
    assert dist[0][lab[0] >= 0].max() == F(np.sqrt(np.float64(F(532684800)))) and F(532684800) == 532684800
    _check_search(oracle, h, 0, 0, Q8, X8, C_, lists, 200, 2, ctx="L2, D 8192")
    h.Close()
    # dot at D = 1024, rows and query all -128: exactly 2^24; and an all-zero row, reported as the flat int8 index reports it
    X8 = rng.integers(-128, 128, (TILE + 3, 1024)).astype(B)
    X8[::5] = -128
    X8[3] = 0
    Q8 = np.full((2, 1024), -128, B)
    Q8[1] = rng.integers(-128, 128, 1024)
    C_ = np.stack([np.full(1024, -100.0, F), np.zeros(1024, F)])
    lists = o8.assign(oracle, 2, 1, X8, C_)
    h = _i8(X8, C_, 2, 1)
    lab, dist = h.search(Q8, 200, 2)
    assert dist[0, 0] == F(-16777216.0) and lab[0, 0] == 0
    _check_search(oracle, h, 2, 1, Q8, X8, C_, lists, 200, 2, ctx="dot, D 1024")
    flat = _flat_i8(X8, 2)
    fl, fd = flat.SearchBatch(Q8, 200)
    assert_same(lab, dist, fl, fd, "dot, D 1024, flat")
    at = np.argwhere(lab == 3)
    assert at.shape[0] == 2 and all(dist[q, j] == 0 for q, j in at)
    assert np.array_equal(np.signbit(dist), np.signbit(fd))
    flat.Close()
    h.Close()


@pytest.mark.parametrize("dim", [4096, 22])
def test_values_dot_one_lane_per_row(oracle, dim):
    """dot over random full-range values in the one-lane-per-row form: at 4096 dimensions, its largest, the four chains reach
    2^24 and their sums round, and at 22 with a tail of two in chain 0; an all-zero row among them"""
    X8, Q8, C_ = _random_case(300, dim, 3, 4, seed=dim + 1)
    X8[:40] = np.where(X8[:40] >= 0, 127, -128)  # (chains near their ends against the queries below)
    X8[7] = 0
    Q8[0] = np.where(X8[0] >= 0, 127, -128)
    Q8[1] = -128
    lists = o8.assign(oracle, 2, 0, X8, C_)
    h = _i8(X8, C_, 2, 0)
    _check_search(oracle, h, 2, 0, Q8, X8, C_, lists, 300, 3, ctx=f"dot, D {dim}")
    flat = _flat_i8(X8, 2)
    lab, dist = h.search(Q8, 300, 3)
    fl, fd = flat.SearchBatch(Q8, 300)
    assert_same(lab, dist, fl, fd, f"dot, D {dim}, flat")
    assert np.array_equal(np.signbit(dist), np.signbit(fd))
    flat.Close()
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def _edge(counts):
    """ivf_oracle.edge_case at 16 dimensions (the staged form) with a noise of one int8 step: rows 100 e_i plus noise, rounded"""
    X, Q, C_, owner = io.edge_case(counts, dim=16, noise=1.0)
    return o8.to_i8(X, 1), o8.to_i8(Q, 1), C_, owner


def test_list_length_edges(oracle):
    counts = (0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
    X8, Q8, C_, owner = _edge(counts)
    lists = o8.assign(oracle, 0, 0, X8, C_)
    assert np.bincount(lists, minlength=len(counts)).tolist() == list(counts) and np.array_equal(lists, owner)
    h = _i8(X8, C_)
    assert np.array_equal(h.assignments(), owner) and h.list_sizes().tolist() == list(counts)
    for nprobe in (1, len(counts)):
        for k in (10, 200, 600):
            _check_search(oracle, h, 0, 0, Q8, X8, C_, owner, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
    lab, dist = h.search(Q8, 10, 1)
    assert (lab[0] == -1).all() and (dist[0] == io.FLT_MAX).all()  # an empty probed list: all padding
    assert lab[1, 0] == np.flatnonzero(owner == 1)[0] and (lab[1, 1:] == -1).all() and (dist[1, 1:] == io.FLT_MAX).all()
    h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_one_workgroup_walks_several_tiles_and_stages(oracle):
    """128 queries x 32 probes = 4,096 pairs, so the scan's grid has one workgroup per (query, list): it walks the three or more
    tiles of a list, three stages each (528 dims: two full and a piece), and the pipeline wraps from a tile's last stage to the
    next tile's first"""
    X8, Q8, C_ = _random_case(16000, 528, 40, 128, seed=528)
    lists = o8.assign(oracle, 0, 0, X8, C_)
    sizes = np.bincount(lists, minlength=40)
    assert np.median(sizes) > 2 * TILE and sizes.max() > 3 * TILE, sizes
    h = _i8(X8, C_)
    assert np.array_equal(h.assignments(), lists)
    _check_search(oracle, h, 0, 0, Q8, X8, C_, lists, 10, 32, ctx="several tiles and stages")
    h.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_skew_and_the_long_selection(oracle):
    X, Q, C_ = io.skew_case(dim=16)
    X8, Q8, C_ = o8.to_i8(X, 20), o8.to_i8(Q, 20), (C_ * F(20)).astype(F)
    lists = o8.assign(oracle, 0, 0, X8, C_)
    assert np.bincount(lists, minlength=4)[0] > LDS_KEYS
    h = _i8(X8, C_)
    assert np.array_equal(h.assignments(), lists)
    for nprobe in (1, 2):
        for k in (1, 2048):
            scanned = _check_search(oracle, h, 0, 0, Q8, X8, C_, lists, k, nprobe, ctx=f"nprobe {nprobe} k {k}")
            assert (scanned > LDS_KEYS).any() and h.last_search_stats()[3] == int((scanned <= LDS_KEYS).sum())
    h.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_adds_in_pieces_with_ids(oracle, parity):
    import torch
    from longbow_amd import ivf
    X8, Q8, C_, lists = parity
    n = X8.shape[0]
    rng = np.random.default_rng(7)
    ids = rng.permutation(1 << 20)[:n].astype(np.int64) + (np.arange(n, dtype=np.int64) % 3 << 41)
    assert np.unique(ids).size == ids.size and (ids > 1 << 40).any()
    one = _i8(X8, C_, ids=ids)
    pieces = _i8(X8[:0], C_)
    dev = _i8(X8[:0], C_)
    dX, dI = torch.from_numpy(X8).cuda(), torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    r0 = 0
    for cnt in (127, 1000, 1873):
        pieces.add(X8[r0:r0 + cnt], ids[r0:r0 + cnt])
        dev.add_device(cnt, dX[r0:].data_ptr(), dI[r0:].data_ptr())
        r0 += cnt
        assert pieces.ntotal == r0 and dev.ntotal == r0
        assert np.array_equal(pieces.assignments(), lists[:r0]) and np.array_equal(dev.assignments(), lists[:r0])
        assert np.array_equal(pieces.list_sizes(), np.bincount(lists[:r0], minlength=C_.shape[0]))
        ol, od, _ = o8.search(oracle, 0, 0, Q8, X8[:r0], C_, lists[:r0], 10, 3, ids=ids[:r0])
        assert_same(*pieces.search(Q8, 10, 3), ol, od, f"host adds, {r0} rows")
        assert_same(*dev.search(Q8, 10, 3), ol, od, f"device-pointer adds, {r0} rows")
    assert r0 == n
    assert_same(*one.search(Q8, 10, 3), ol, od, "one add, ids")
    assert np.array_equal(dev.list_sizes(), one.list_sizes())
    # ids on every add or on none, as on a float32 handle
    for h, bad in ((pieces, None), (_i8(X8[:5], C_), ids[:3])):
        before = h.ntotal
        rc = h._lib.lb_gpu_ivf_add_i8(h._h, 3, X8.ctypes.data, bad.ctypes.data if bad is not None else None)
        assert rc == INVALID and h.ntotal == before
        with pytest.raises(ivf._lib.LongbowGPUError, match="ids"):
            h.add(X8[:3], bad)
        assert h.ntotal == before
        if h is not pieces:
            h.Close()
    assert_same(*pieces.search(Q8, 10, 3), ol, od, "after the refused add")
    for h in (one, pieces, dev):
        h.Close()


def test_an_add_that_crosses_the_assignment_piece():
    """65,536 + 300 rows in one add: the rows are widened and assigned in two pieces"""
    n = 65536 + 300
    X8, Q8, C_ = _random_case(n, 8, 4, 5, seed=65)
    h8, h32 = _i8(X8, C_), _f32(X8.astype(F), C_)
    assert h8.ntotal == n
    assert np.array_equal(h8.assignments(), h32.assignments())
    assert np.array_equal(h8.list_sizes(), h32.list_sizes())
    flat = _flat_i8(X8, 0)
    assert_same(*h8.search(Q8, 10, 4), *flat.SearchBatch(Q8, 10), "65,836 rows, every list")
    for x in (flat, h8, h32):
        x.Close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_filters_at_the_tile_edges(oracle):
    X8, Q8, C_, owner = _edge(fc.EDGE_COUNTS)
    assert np.array_equal(o8.assign(oracle, 0, 0, X8, C_), owner)
    mask = fc.keep_per_list(owner, fc.EDGE_KEEP)
    h = _i8(X8, C_)
    h.set_filter(mask)
    assert h.nvisible() == sum(fc.EDGE_KEEP) and h.list_sizes().tolist() == list(fc.EDGE_COUNTS)
    for nprobe in (1, 2, len(fc.EDGE_COUNTS)):
        scanned = _check_search(oracle, h, 0, 0, Q8, X8, C_, owner, fc.K, nprobe, mask=mask, ctx=f"nprobe {nprobe}")
        if nprobe == 1:
            assert scanned.tolist() == list(fc.EDGE_KEEP)
    h.Close()


def test_filter_column_an_add_under_a_filter_and_clearing(oracle, parity):
    X8, Q8, C_, lists = parity
    n = X8.shape[0]
    rng = np.random.default_rng(17)
    col = rv.int64_edge_column(n)
    fcol = rv.float32_edge_column(n)
    valid = rng.random(n) < 0.8

    def check(h, rows, mask, ctx):
        assert h.nvisible() == np.count_nonzero(mask), ctx
        _check_search(oracle, h, 0, 0, Q8, X8[:rows], C_, lists[:rows], fc.K, 3, mask=mask, ctx=ctx)

    h = _i8(X8[:1000], C_)
    h.filter_column(col[:1000], 2 ** 32, rv.GE, valid=rv.validity_bitmap(valid[:1000], 3), validity_offset=3)
    m = rv.predicate(col[:1000], 2 ** 32, rv.GE, valid[:1000])
    assert 0 < np.count_nonzero(m) < 1000
    check(h, 1000, m, "filter_column, int64 with a validity bitmap")
    h.filter_column(fcol[:1000], 0.25, rv.LE, combine=True)
    m2 = rv.and_bytes(m, rv.predicate(fcol[:1000], 0.25, rv.LE))
    assert 0 < np.count_nonzero(m2) < np.count_nonzero(m)
    check(h, 1000, m2, "filter_column, float32 combined")
    h.add(X8[1000:])  # the new rows are visible
    full = np.concatenate([m2, np.ones(n - 1000, np.uint8)])
    assert h.ntotal == n and np.array_equal(h.assignments(), lists)
    check(h, n, full, "an add under a filter")
    h.reserve(20000)  # a change of capacity keeps the filter and the int8 rows
    check(h, n, full, "after reserve")
    h.set_filter(None)
    assert h.nvisible() == n
    _check_search(oracle, h, 0, 0, Q8, X8, C_, lists, 10, 3, ctx="filter cleared")
    h.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_device_pointers(oracle, parity):
    """add_i8_device and search_i8_device_ctx through torch tensors; queries at an odd byte offset take the one-lane-per-row
    form; every slot of the pre-filled outputs is written"""
    import torch
    X8, Q8, C_, lists = parity
    h = _i8(X8[:0], C_, 2, 1)
    dX = torch.from_numpy(X8).cuda()
    torch.cuda.synchronize()
    h.add_device(X8.shape[0], dX.data_ptr())
    lists = o8.assign(oracle, 2, 1, X8, C_)
    assert np.array_equal(h.assignments(), lists)
    nq, dim = Q8.shape
    buf = torch.zeros(nq * dim + 16, dtype=torch.int8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dQ = torch.from_numpy(Q8).cuda()
    buf[1:1 + nq * dim] = dQ.reshape(-1)
    k = 40
    ol, od, _ = o8.search(oracle, 2, 1, Q8, X8, C_, lists, k, 1)
    for ptr in (dQ.data_ptr(), buf.data_ptr() + 1):
        dD = torch.full((nq, k), -5.0, dtype=torch.float32, device="cuda")
        dL = torch.full((nq, k), -5, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        h.search_device(nq, ptr, k, 1, dD.data_ptr(), dL.data_ptr())
        assert_same(dL.cpu().numpy(), dD.cpu().numpy(), ol, od, f"queries at {ptr % 16} mod 16")
    assert dQ.data_ptr() % 16 == 0
    h.Close()


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_refusals_behind_a_live_handle(oracle, parity):
    import torch
    from longbow_amd import gpu, ivf
    from longbow_amd.gpu import DataType
    X8, Q8, C_, lists = parity
    W, WQ = X8.astype(F), Q8.astype(F)
    H16 = X8.astype(np.float16)
    h8, h32, h16 = _i8(X8[:500], C_), _f32(W[:500], C_), ivf.IVFFlat(C_, dtype=DataType.Float16)
    h16.add(H16[:500])
    lib = h8._lib
    nq = Q8.shape[0]
    dist = np.full((nq, LB_MAX_K + 1), 9.0, F)
    lab = np.full((nq, LB_MAX_K + 1), 77, np.int64)
    dW, dH, dB = torch.from_numpy(W[:3].copy()).cuda(), torch.from_numpy(H16[:3].copy()).cuda(), torch.from_numpy(X8[:3].copy()).cuda()
    dD = torch.full((nq, 10), 9.0, dtype=torch.float32, device="cuda")
    dL = torch.full((nq, 10), 77, dtype=torch.int64, device="cuda")
    dQ8, dQ = torch.from_numpy(Q8).cuda(), torch.from_numpy(WQ).cuda()
    torch.cuda.synchronize()
    out = (dist.ctypes.data, lab.ctypes.data)
    for n in (3, 0):
        # an f32 or _f16 add, or an f32 search, on an int8 handle
        assert lib.lb_gpu_ivf_add(h8._h, n, W.ctypes.data, None) == INVALID
        assert b"int8" in lib.lb_gpu_ivf_last_error(h8._h)
        assert lib.lb_gpu_ivf_add_device(h8._h, n, dW.data_ptr(), None) == INVALID
        assert lib.lb_gpu_ivf_add_f16(h8._h, n, H16.ctypes.data, None) == INVALID
        assert lib.lb_gpu_ivf_add_f16_device(h8._h, n, dH.data_ptr(), None) == INVALID
        assert lib.lb_gpu_ivf_search(h8._h, n, WQ.ctypes.data, 10, 3, *out) == INVALID
        assert lib.lb_gpu_ivf_search_ctx(h8._h, n, WQ.ctypes.data, 10, 3, *out, None) == INVALID
        assert lib.lb_gpu_ivf_search_device_ctx(h8._h, n, dQ.data_ptr(), 10, 3, dD.data_ptr(), dL.data_ptr(), None, None) == INVALID
        assert b"int8" in lib.lb_gpu_ivf_last_error(h8._h)
        # an _i8 add or search on a float32 or float16 handle
        for h, name in ((h32, b"float32"), (h16, b"float16")):
            assert lib.lb_gpu_ivf_add_i8(h._h, n, X8.ctypes.data, None) == INVALID
            assert name in lib.lb_gpu_ivf_last_error(h._h)
            assert lib.lb_gpu_ivf_add_i8_device(h._h, n, dB.data_ptr(), None) == INVALID
            assert lib.lb_gpu_ivf_search_i8(h._h, n, Q8.ctypes.data, 10, 3, *out) == INVALID
            assert lib.lb_gpu_ivf_search_i8_ctx(h._h, n, Q8.ctypes.data, 10, 3, *out, None) == INVALID
            assert lib.lb_gpu_ivf_search_i8_device_ctx(h._h, n, dQ8.data_ptr(), 10, 3, dD.data_ptr(), dL.data_ptr(), None, None) == INVALID
            assert name in lib.lb_gpu_ivf_last_error(h._h)
    assert h8.ntotal == 500 and h32.ntotal == 500 and h16.ntotal == 500
    with pytest.raises(TypeError):
        h8.add(W[:3])  # (float32 data is not converted silently)
    with pytest.raises(TypeError):
        h8.search(WQ, 10, 3)
    # k and nprobe, as on the float32 handle
    args = (nq, Q8.ctypes.data)
    assert lib.lb_gpu_ivf_search_i8(h8._h, *args, LB_MAX_K + 1, 3, *out) == UNSUPPORTED
    assert b"2048" in lib.lb_gpu_ivf_last_error(h8._h)
    assert lib.lb_gpu_ivf_search_i8(h8._h, *args, 10, 0, *out) == INVALID
    assert b"nprobe" in lib.lb_gpu_ivf_last_error(h8._h)
    assert lib.lb_gpu_ivf_search_i8(h8._h, *args, 10, -4, *out) == INVALID
    assert lib.lb_gpu_ivf_search_i8(h8._h, *args, 0, 3, *out) == INVALID
    c = gpu.Cancel()
    c.fire()
    assert lib.lb_gpu_ivf_search_i8_ctx(h8._h, *args, 10, 3, *out, c._h) == CANCELLED
    assert lib.lb_gpu_ivf_search_i8_device_ctx(h8._h, nq, dQ8.data_ptr(), 10, 3, dD.data_ptr(), dL.data_ptr(), None, c._h) == CANCELLED
    torch.cuda.synchronize()
    assert (dist == 9.0).all() and (lab == 77).all() and bool((dD == 9.0).all()) and bool((dL == 77).all())
    assert h8.ntotal == 500
    _check_search(oracle, h8, 0, 0, Q8, X8[:500], C_, lists[:500], 10, 3, ctx="after the refused calls")
    for h in (h8, h32, h16):
        h.Close()


# 12 --------------------------------------------------------------------------------------------------------------------------
def test_bytes():
    from longbow_amd import ivf
    from longbow_amd.gpu import DataType
    C_ = np.eye(4, 16, dtype=F)
    h8, h16 = _i8(np.empty((0, 16), B), C_), ivf.IVFFlat(C_, dtype=DataType.Float16)
    assert h8.hbm_bytes == h16.hbm_bytes
    h8.reserve(5000)
    h16.reserve(5000)
    assert h16.hbm_bytes - h8.hbm_bytes == 5000 * 16  # the rows term: n * D against 2 * n * D
    h8.Close()
    h16.Close()


# 13 --------------------------------------------------------------------------------------------------------------------------
def test_python_mirror(oracle, parity):
    from longbow_amd import ivf
    gpu_or_skip()
    X8, Q8, C_, lists = parity
    n = X8.shape[0]
    ids = np.arange(n, dtype=np.int64) * 7 + (1 << 33)
    h = ivf.IVFFlatInt8(C_, metric=0, order=1)
    assert (h.dtype, h.ntotal, h.nlist, h.dims, h.metric, h.order) == (2, 0, 16, 16, 0, 1)
    lab, dist = h.search(Q8, 5, 3)
    assert (lab == -1).all() and (dist == io.FLT_MAX).all()  # an empty handle: all padding
    h.add(X8[:2000], ids[:2000])
    h.add(X8[2000:], ids[2000:])
    lists1 = o8.assign(oracle, 0, 1, X8, C_)
    assert np.array_equal(h.assignments(), lists1) and np.array_equal(h.centroids(), C_)
    _check_search(oracle, h, 0, 1, Q8, X8, C_, lists1, 10, 3, ids=ids, ctx="with ids")
    h.set_profiling(True)
    h.search(Q8, 10, 3)
    h.set_filter(np.ones(n, np.uint8))
    h.set_profiling(False)
    t = h.last_timing()
    assert len(t) == 4 and all(x >= 0 for x in t) and t[2] > 0 and h.last_build_timing() > 0
    assert h.hbm_bytes >= X8.nbytes + C_.nbytes
    h.Close()
    h.Close()
