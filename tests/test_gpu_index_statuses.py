"""What the flat index's entry points answer before they touch the device, and what a refused allocation leaves behind.

The status of every argument combination below, and the lb_gpu_last_error text where one is set, were read off the code before
the entry points moved into the shared shell (lb_handle.h: guard, knn_args) and are asserted unchanged.  The three assertions
that name an intended change of that move are marked INTENDED CHANGE.  Corpus: 100 rows x 16 dims, k = 5."""
import threading
import time

import numpy as np
import pytest

from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
N, D, K = 100, 16, 5
MAX_K = 2048
OK, INVALID, HIP, OOM, UNSUPPORTED, CANCELLED, DEADLINE = 0, 1, 4, 5, 6, 8, 9
TAGS = {0: "", 1: "_f16", 2: "_i8"}
NP = {0: np.float32, 1: np.float16, 2: np.int8}
HOLDS = {0: "this index holds float32 rows: use the float32 entry point",
         1: "this index holds float16 rows: use the _f16 entry point",
         2: "this index holds int8 rows: use the _i8 entry point"}


def rows_of(dtype, n=N, seed=7):
    rng = np.random.default_rng(seed + dtype)
    if dtype == 2:
        return rng.integers(-100, 100, (n, D)).astype(np.int8)
    return rng.random((n, D), dtype=F).astype(NP[dtype])


def new_index(dtype):
    from longbow_amd import gpu
    return gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=D, Metric=0, DataType=dtype))


def last_error(lib, idx):
    return lib.lb_gpu_last_error(idx._h).decode()


@pytest.fixture(scope="module")
def indexes():
    """one f32, one fp16 and one int8 index of the same shape; the statuses tests change none of them"""
    gpu_or_skip()
    out = {}
    for dtype in (0, 1, 2):
        idx = new_index(dtype)
        idx.Add(None, rows_of(dtype))
        out[dtype] = idx
    yield out
    for idx in out.values():
        idx.Close()


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_search_statuses(indexes, dtype, device):
    import torch
    from longbow_amd import gpu
    lib = gpu_or_skip()
    idx = indexes[dtype]
    h = idx._h
    q_host = rows_of(dtype, 1, seed=99)
    dist_host, lab_host = np.zeros(K, F), np.zeros(K, np.int64)
    if device:
        q_dev = torch.from_numpy(q_host).cuda()
        dist_dev, lab_dev = torch.zeros(K, device="cuda"), torch.zeros(K, dtype=torch.int64, device="cuda")
        q, dist, lab = q_dev.data_ptr(), dist_dev.data_ptr(), lab_dev.data_ptr()
    else:
        q, dist, lab = q_host.ctypes.data, dist_host.ctypes.data, lab_host.ctypes.data

    def entry(tag):
        fn = getattr(lib, "lb_gpu_index_search" + tag + ("_device_ctx" if device else "_ctx"))
        if device:
            return lambda h_, nq, q_, k, d_, l_, ctx=None: fn(h_, nq, q_, k, d_, l_, None, ctx)
        return lambda h_, nq, q_, k, d_, l_, ctx=None: fn(h_, nq, q_, k, d_, l_, ctx)

    search = entry(TAGS[dtype])
    other = (dtype + 1) % 3
    wrong = entry(TAGS[other])  # the entry point of another element type

    # null pointers and negative counts: LB_ERR_INVALID_ARG
    assert search(None, 1, q, K, dist, lab) == INVALID
    assert search(h, 1, None, K, dist, lab) == INVALID
    assert search(h, 1, q, K, None, lab) == INVALID
    assert search(h, 1, q, K, dist, None) == INVALID
    assert search(h, -1, q, K, dist, lab) == INVALID
    assert search(h, 1, q, 0, dist, lab) == INVALID
    assert search(h, 1, q, -3, dist, lab) == INVALID
    assert search(h, 0, None, 0, None, None) == INVALID
    assert wrong(h, -1, q, K, dist, lab) == INVALID          # (before the element type)
    # the wrong element type: LB_ERR_INVALID_ARG with the text, before k is looked at
    assert wrong(h, 1, q, K, dist, lab) == INVALID
    assert last_error(lib, idx) == HOLDS[dtype]
    assert wrong(h, 1, q, MAX_K + 1, dist, lab) == INVALID
    # no queries: LB_OK, k is not looked at; the device entry points look at the element type first, the host ones do not
    assert search(h, 0, None, MAX_K + 1, None, None) == OK
    assert search(h, 0, q, K, dist, lab) == OK
    assert wrong(h, 0, None, K, None, None) == (INVALID if device else OK)
    # k beyond LB_MAX_K: LB_ERR_UNSUPPORTED
    assert search(h, 1, q, MAX_K + 1, dist, lab) == UNSUPPORTED
    assert last_error(lib, idx) == f"k={MAX_K + 1} exceeds the supported maximum {MAX_K}"
    # the context, last: a fired token, a deadline that has passed
    c = gpu.Cancel()
    c.fire()
    c2 = gpu.Cancel(deadline_ms=0)
    time.sleep(0.002)
    assert search(h, 1, q, K, dist, lab, c._h) == CANCELLED
    assert last_error(lib, idx) == "context canceled"
    assert search(h, 1, q, K, dist, lab, c2._h) == DEADLINE
    assert last_error(lib, idx) == "context deadline exceeded"
    assert search(h, 1, q, MAX_K + 1, dist, lab, c._h) == UNSUPPORTED   # (k before the context)
    assert wrong(h, 1, q, K, dist, lab, c._h) == INVALID                 # (the element type before the context)
    assert search(h, 0, None, K, None, None, c._h) == OK                 # (no queries: the context is not looked at)
    # a live context and a good call: the answer, identical through both entry points' neighbours
    c3 = gpu.Cancel(deadline_ms=60_000)
    assert search(h, 1, q, K, dist, lab, c3._h) == OK
    got = (lab_dev.cpu().numpy(), dist_dev.cpu().numpy()) if device else (lab_host.copy(), dist_host.copy())
    want = idx.SearchBatch(q_host, K)
    assert np.array_equal(got[0], want[0][0]) and np.array_equal(got[1], want[1][0])
    for c_ in (c, c2, c3):
        c_.close()


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_add_statuses(dtype):
    import torch
    lib = gpu_or_skip()
    idx = new_index(dtype)
    h = idx._h
    X = rows_of(dtype)
    Xd = torch.from_numpy(X).cuda()
    other = (dtype + 1) % 3
    for suffix, ptr in (("", X.ctypes.data), ("_device", Xd.data_ptr())):
        add = getattr(lib, "lb_gpu_index_add" + TAGS[dtype] + suffix)
        wrong = getattr(lib, "lb_gpu_index_add" + TAGS[other] + suffix)
        assert add(None, N, ptr, None) == INVALID
        assert add(h, -1, ptr, None) == INVALID
        assert add(h, N, None, None) == INVALID
        assert wrong(h, N, ptr, None) == INVALID
        assert last_error(lib, idx) == HOLDS[dtype]
        assert wrong(h, 0, None, None) == INVALID     # (the element type before "no rows")
        assert add(h, 0, None, None) == OK
        assert lib.lb_gpu_index_ntotal(h) == (0 if suffix == "" else N)
        assert add(h, N, ptr, None) == OK
    assert lib.lb_gpu_index_ntotal(h) == 2 * N
    q = rows_of(dtype, 3, seed=5)
    lab, dist = idx.SearchBatch(q, K)
    assert np.array_equal(lab[:, 0] % N, lab[:, 1] % N) and np.array_equal(dist[:, 0], dist[:, 1])  # (the same rows, twice)
    idx.Close()


def test_rerank_statuses(indexes):
    import torch
    lib = gpu_or_skip()
    idx = indexes[0]
    h = idx._h
    q = rows_of(0, 1, seed=3)[0]
    rows = np.array([3, 99, -1, 100, 0], np.int64)
    dist, score = np.zeros(rows.size, F), np.zeros(rows.size, F)
    rr = lib.lb_gpu_index_rerank
    assert rr(None, q.ctypes.data, rows.ctypes.data, rows.size, 1, dist.ctypes.data, score.ctypes.data) == INVALID
    assert rr(h, q.ctypes.data, rows.ctypes.data, -1, 1, dist.ctypes.data, score.ctypes.data) == INVALID
    assert rr(h, None, None, 0, 1, None, None) == OK
    assert rr(h, None, rows.ctypes.data, rows.size, 1, dist.ctypes.data, score.ctypes.data) == INVALID
    assert rr(h, q.ctypes.data, None, rows.size, 1, dist.ctypes.data, score.ctypes.data) == INVALID
    assert rr(h, q.ctypes.data, rows.ctypes.data, rows.size, 1, None, score.ctypes.data) == INVALID
    assert rr(h, q.ctypes.data, rows.ctypes.data, rows.size, 5, dist.ctypes.data, score.ctypes.data) == INVALID  # (order)
    assert rr(h, q.ctypes.data, rows.ctypes.data, rows.size, 1, dist.ctypes.data, None) == OK
    dq, drows = torch.from_numpy(q).cuda(), torch.from_numpy(rows).cuda()
    dd, ds = torch.zeros(rows.size, device="cuda"), torch.zeros(rows.size, device="cuda")
    rd = lib.lb_gpu_index_rerank_device
    assert rd(None, dq.data_ptr(), drows.data_ptr(), rows.size, 1, dd.data_ptr(), ds.data_ptr(), None) == INVALID
    assert rd(h, dq.data_ptr(), drows.data_ptr(), -1, 1, dd.data_ptr(), ds.data_ptr(), None) == INVALID
    assert rd(h, dq.data_ptr(), drows.data_ptr(), rows.size, 7, dd.data_ptr(), ds.data_ptr(), None) == INVALID
    assert rd(h, None, None, 0, 1, None, None, None) == OK
    assert rd(h, None, drows.data_ptr(), rows.size, 1, dd.data_ptr(), ds.data_ptr(), None) == INVALID
    assert rd(h, dq.data_ptr(), None, rows.size, 1, dd.data_ptr(), ds.data_ptr(), None) == INVALID
    assert rd(h, dq.data_ptr(), drows.data_ptr(), rows.size, 1, None, ds.data_ptr(), None) == INVALID
    assert rd(h, dq.data_ptr(), drows.data_ptr(), 2**31, 1, dd.data_ptr(), ds.data_ptr(), None) == INVALID
    # a good call through both: the same distances, MaxFloat32 / 0 for the rows outside the corpus
    assert rr(h, q.ctypes.data, rows.ctypes.data, rows.size, 1, dist.ctypes.data, score.ctypes.data) == OK
    assert rd(h, dq.data_ptr(), drows.data_ptr(), rows.size, 1, dd.data_ptr(), ds.data_ptr(), None) == OK
    assert np.array_equal(dd.cpu().numpy(), dist) and np.array_equal(ds.cpu().numpy(), score)
    assert dist[2] == dist[3] == np.finfo(F).max and score[2] == score[3] == 0
    # not on an fp16 or int8 index: LB_ERR_UNSUPPORTED with the text
    for dtype, name in ((1, "float16"), (2, "int8")):
        o = indexes[dtype]
        assert rr(o._h, q.ctypes.data, rows.ctypes.data, rows.size, 1, dist.ctypes.data, score.ctypes.data) == UNSUPPORTED
        assert last_error(lib, o) == f"re-rank reads float32 rows: not available on a {name} index"
        assert rd(o._h, dq.data_ptr(), drows.data_ptr(), rows.size, 1, dd.data_ptr(), ds.data_ptr(), None) == UNSUPPORTED
        assert last_error(lib, o) == f"re-rank reads float32 rows: not available on a {name} index"


def test_filter_statuses(oracle):
    lib = gpu_or_skip()
    idx = new_index(0)
    X = rows_of(0)
    idx.Add(None, X)
    h = idx._h
    mask = np.ones(N, np.uint8)
    col = np.arange(N, dtype=np.int64)
    colf = np.arange(N, dtype=F)
    assert lib.lb_gpu_index_set_filter(None, mask.ctypes.data, N) == INVALID
    assert lib.lb_gpu_index_set_filter(h, mask.ctypes.data, 5) == INVALID
    assert last_error(lib, idx) == f"filter mask has 5 bytes, index has {N} rows"
    assert lib.lb_gpu_index_set_filter(h, None, 0) == OK
    for fn, c, v in ((lib.lb_gpu_index_filter_int64, col, 50), (lib.lb_gpu_index_filter_float32, colf, 50.0)):
        assert fn(None, c.ctypes.data, N, v, 0, None, 0, 0) == INVALID
        assert fn(h, c.ctypes.data, N, v, 6, None, 0, 0) == INVALID
        assert fn(h, c.ctypes.data, N, v, -1, None, 0, 0) == INVALID
        assert fn(h, c.ctypes.data, N, v, 0, None, -1, 0) == INVALID
        assert fn(h, c.ctypes.data, 5, v, 0, None, 0, 0) == INVALID
        assert last_error(lib, idx) == f"filter column has 5 values, index has {N} rows"
        assert fn(h, None, N, v, 0, None, 0, 0) == INVALID
        assert last_error(lib, idx) == f"filter column has {N} values, index has {N} rows"
    # none of the refused calls left a filter behind
    q = rows_of(0, 2, seed=11)
    lab, dist = idx.SearchBatch(q, K)
    oi, od = oracle.search_batch(0, q, X, K, nthreads=2)
    assert_same(lab, dist, oi, od, "after refused filter calls")
    idx.Close()


def test_filter_column_refused_in_the_body_leaves_the_index_usable(oracle):
    """filter_int64 with a validity bitmap at an offset of 2^62 bits: the bitmap's device copy would be 2^59 bytes, one pool
    allocation (BufPool::get: one hipMalloc of the rounded size, asserted below to be beyond the device's whole memory) that
    the allocator refuses by its size; the host bitmap is never read (the copy comes after the lease).  The column's copy is
    already enqueued by then: the call answers LB_ERR_OOM with the text, and the index filters and searches as before."""
    import torch
    lib = gpu_or_skip()
    idx = new_index(0)
    X = rows_of(0)
    idx.Add(None, X)
    col = np.arange(N, dtype=np.int64)
    validity = np.full(16, 0xFF, np.uint8)
    voff = 1 << 62
    assert (voff + N + 7) // 8 > torch.cuda.mem_get_info(0)[1]
    assert lib.lb_gpu_index_filter_int64(idx._h, col.ctypes.data, N, 50, 4, validity.ctypes.data, voff, 0) == OOM  # op 4: <
    assert last_error(lib, idx) == "HIP error 2 (out of memory) in hipMalloc (pool)"
    q = rows_of(0, 2, seed=12)
    oi, od = oracle.search_batch(0, q, X, K, nthreads=2)
    lab, dist = idx.SearchBatch(q, K)
    assert_same(lab, dist, oi, od, "after the refused filter")       # (no filter was left behind)
    idx.filter_column(col, "<", 50, validity=validity, validity_offset=3)
    lab, dist = idx.SearchBatch(q, K)
    oi, od = oracle.search_batch(0, q, X[:50], K, nthreads=2)
    assert_same(lab, dist, oi, od, "the same filter at a sane offset")
    idx.Close()


def test_refused_reservation_leaves_thread_and_handle_usable(oracle):
    """lb_gpu_*_reserve of more rows than the device has bytes for, then an add and a search on the same thread and handle.
    Every request is refused by its size and never attempted in part, checked by reading the code: the flat index's goes to
    VmmBuf::ensure, which compares it with the reserved range (the device's memory) and throws before any driver call (without
    the mapped corpus: one hipMalloc of it); the code handles' *_grow make one hipMalloc (DevBuf::alloc) of the whole buffer
    first.  Each size is asserted to be beyond the device's whole memory."""
    import torch
    from longbow_amd import bq, pq, sq8
    lib = gpu_or_skip()
    total = torch.cuda.mem_get_info(0)[1]
    rng = np.random.default_rng(77)

    # the flat index
    idx = new_index(0)
    X = rows_of(0)
    big = 1 << 40
    assert big * D * 4 > total
    assert lib.lb_gpu_index_reserve(idx._h, big) == OOM
    assert last_error(lib, idx) != ""
    idx.Add(None, X)
    q = rows_of(0, 2, seed=13)
    lab, dist = idx.SearchBatch(q, K)
    oi, od = oracle.search_batch(0, q, X, K, nthreads=2)
    assert_same(lab, dist, oi, od, "flat index after the refused reservation")
    idx.Close()

    # BQ: 8192 dims = 1 KiB a code, 2^31 - 1 codes
    d = 8192
    S = rng.random((N, d), dtype=F) - F(0.5)
    benc = bq.BQEncoder(d)
    big = (1 << 31) - 1
    assert big * (d // 8) > total
    assert lib.lb_gpu_bq_reserve(benc._h, big) == OOM
    assert lib.lb_gpu_bq_last_error(benc._h).decode() != ""
    codes = benc.Encode(S)                       # INTENDED CHANGE 1: the thread's next calls are LB_OK (a launch check in them
    benc.add_codes(codes)                        # used to find the refused hipMalloc as HIP's last error)
    lab, dist = benc.search(S[:2], K)
    for b in range(2):
        hd = np.bitwise_count(codes ^ codes[b]).sum(axis=1)
        oi = np.lexsort((np.arange(hd.size), hd))[:K]
        assert np.array_equal(lab[b], oi) and np.array_equal(dist[b], hd[oi].astype(F))
    benc.Close()

    # SQ8: 8192 dims = 8 KiB a code
    senc = sq8.train(S)
    assert big * d > total
    assert lib.lb_gpu_sq8_reserve(senc._h, big) == OOM
    assert lib.lb_gpu_sq8_last_error(senc._h).decode() != ""
    scodes = senc.Encode(S)                      # INTENDED CHANGE 1, as above
    senc.add_codes(scodes)
    lab, dist = senc.search_codes(scodes[:2], K)
    for b in range(2):
        df = scodes.astype(np.int64) - scodes[b].astype(np.int64)
        s2 = (df * df).sum(axis=1)
        oi = np.lexsort((np.arange(s2.size), s2))[:K]
        assert np.array_equal(lab[b], oi) and np.array_equal(dist[b], s2[oi].astype(F))
    senc.Close()

    # PQ: 8 bytes a code, 2^50 codes (the PQ handle takes more than 2^31 rows without a filter)
    M, dims = 8, 32
    cb = rng.random((M, 256, dims // M), dtype=F)
    enc = pq.PQEncoder(pq.serialize_codebooks(cb))
    big = 1 << 50
    assert big * M > total
    assert lib.lb_gpu_pq_reserve(enc._h, big) == OOM
    assert lib.lb_gpu_pq_last_error(enc._h).decode() != ""
    pcodes = rng.integers(0, 256, (N, M), dtype=np.uint8)
    enc.add_codes(pcodes)                        # INTENDED CHANGE 1, as above
    Q = rng.random((2, dims), dtype=F)
    lab, dist = enc.Search(Q, K)
    for b in range(2):
        oi, od, _ = oracle.topk_canonical(oracle.adc_batch(oracle.build_adc_table(cb, Q[b]), pcodes), K)
        assert np.array_equal(lab[b], oi) and np.array_equal(dist[b], od)
    enc.Close()


def test_concurrent_pq_host_searches_are_combined_and_identical():
    """Eight threads of single-query host searches on a small PQ handle (4,096 codes, 32 dims, M = 8): every answer is the
    uncombined answer bit for bit, and the counters count the combined batches.  (The flat index's half of this is
    test_gpu_hardening.py::test_concurrent_single_query_searches_are_combined_and_identical.)"""
    from longbow_amd import pq
    gpu_or_skip()
    rng = np.random.default_rng(4096)
    M, dims, n = 8, 32, 4096
    cb = rng.random((M, 256, dims // M), dtype=F)
    enc = pq.PQEncoder(pq.serialize_codebooks(cb))
    enc.add_codes(rng.integers(0, 256, (n, M), dtype=np.uint8))
    Q = rng.random((64, dims), dtype=F)
    enc.set_search_combining(False)
    want = [enc.Search(Q[i], K) for i in range(len(Q))]
    assert enc.combining_stats == (0, 0)
    enc.set_search_combining(True)
    errors = []

    def caller(t):
        try:
            for rep in range(40):
                for i in range(t, len(Q), 8):
                    lab, dist = enc.Search(Q[i], K)
                    if not (np.array_equal(lab, want[i][0]) and np.array_equal(dist, want[i][1])):
                        errors.append(f"thread {t} query {i} rep {rep}: differs from the search on its own")
        except Exception as e:  # noqa: BLE001
            errors.append(f"thread {t}: {type(e).__name__}: {e}")

    ths = [threading.Thread(target=caller, args=(t,)) for t in range(8)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errors, errors[:5]
    batches, requests = enc.combining_stats
    assert batches > 0 and requests >= 2 * batches, (batches, requests)
    enc.Close()
