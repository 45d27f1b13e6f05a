"""int8 index on the device: signed int8 rows, results equal to the reference's int8 registry kernels bit for bit
(tests/i8_oracle.py; tests/test_i8_semantics.py pins the oracle to line-for-line transcriptions)."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import i8_oracle as io
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu

F, I8 = np.float32, np.int8
L2, COS, DOT = 0, 1, 2
ROUTE_I8_SCAN, ROUTE_I8_MFMA = 80, 81


def mfma_expected(metric, dim, nq, n):
    """the batches the i8 MFMA pass serves: from 16 queries, D % 16 == 0 (dot: D <= 1024), a sampled threshold (n >= 16,384)"""
    return nq >= 16 and dim % 16 == 0 and (metric == L2 or dim <= 1024) and n >= 16384


def new_i8(dim, metric):
    from longbow_amd import gpu
    return gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=dim, Metric=metric, DataType=gpu.DataType.Int8))


def rows(rng, n, dim):
    return rng.integers(-128, 128, (n, dim), dtype=np.int64).astype(I8)


@pytest.mark.parametrize("metric", [L2, DOT])
@pytest.mark.parametrize("dim", [7, 16, 100, 128, 768, 1536])
def test_i8_grid(metric, dim):
    gpu_or_skip()
    rng = np.random.default_rng(dim * 3 + metric)
    n = 20000
    X = rows(rng, n, dim)
    X[5:9] = X[100]  # duplicate rows: ties broken by row
    X[200] = 127
    X[201] = -128
    X[202] = 0
    Q = rows(rng, 1024, dim)
    Q[1] = X[100]
    Q[2] = -128
    idx = new_i8(dim, metric)
    try:
        idx.Add(None, X)
        assert idx.dtype() == 2 and idx.f16_image_bytes == 0
        D = io.distances(metric, Q, X)  # every (query, row) once; the batches below are prefixes
        for nq in (1, 3, 64, 200, 1024):
            for k in (1, 10, 100, 1000):
                if nq * k > 200 * 1000:
                    continue  # (the oracle's share of the run time)
                lab, dist = idx.SearchBatch(Q[:nq], k)
                for q in range(nq):
                    oi, od = io.topk(D[q], k)
                    assert_same(lab[q], dist[q], oi, od, f"metric {metric} dim {dim} nq {nq} k {k} query {q}")
                route = idx._lib.lb_gpu_index_last_route(idx._h)
                if k <= 100:  # (k = 1000 over 20,000 rows: the sampled span ends short of the corpus, the scan serves it)
                    assert route == (ROUTE_I8_MFMA if mfma_expected(metric, dim, nq, n) else ROUTE_I8_SCAN), (nq, k, route)
                else:
                    assert route in (ROUTE_I8_SCAN, ROUTE_I8_MFMA)
    finally:
        idx.Close()


@pytest.mark.parametrize("metric", [L2, DOT])
def test_small_corpus_constant_rows_and_extremes(metric):
    gpu_or_skip()
    dim = 64
    X = np.zeros((300, dim), I8)
    X[::3] = 127
    X[1::3] = -128
    X[50:60] = 5  # constant rows, equal to each other
    Q = np.stack([np.full(dim, 127, I8), np.full(dim, -128, I8), np.zeros(dim, I8), np.full(dim, 5, I8)])
    idx = new_i8(dim, metric)
    try:
        idx.Add(None, X)
        for k in (1, 10, 100, 1000):  # (k beyond the corpus: -1 / FLT_MAX padding)
            lab, dist = idx.SearchBatch(Q, k)
            oi, od = io.search(metric, Q, X, k)
            assert_same(lab, dist, oi, od, f"k {k}")
    finally:
        idx.Close()


def test_order_is_accepted_and_changes_nothing():
    gpu_or_skip()
    rng = np.random.default_rng(5)
    X, Q = rows(rng, 5000, 100), rows(rng, 8, 100)
    idx = new_i8(100, L2)
    try:
        idx.Add(None, X)
        a = idx.SearchBatch(Q, 10)
        idx.set_order(0)
        b = idx.SearchBatch(Q, 10)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        lab, dist = idx.Search(Q[0], 10)
        assert np.array_equal(lab, a[0][0]) and np.array_equal(dist, a[1][0])
    finally:
        idx.Close()


def _filter_int64(idx, col, value, op):
    col = np.ascontiguousarray(col, np.int64)
    return idx._lib.lb_gpu_index_filter_int64(idx._h, col.ctypes.data, col.size, int(value), op, None, 0, 0)


@pytest.mark.parametrize("metric", [L2, DOT])
def test_ids_several_adds_reserve_and_masks(metric):
    gpu_or_skip()
    rng = np.random.default_rng(17 + metric)
    dim = 128
    X = rows(rng, 40000, dim)
    ids = rng.permutation(10 ** 6)[:40000].astype(np.int64)
    Q = rows(rng, 70, dim)
    idx = new_i8(dim, metric)
    try:
        idx.reserve(50000)
        for a, b in ((0, 1000), (1000, 17000), (17000, 40000)):
            idx.Add(ids[a:b], X[a:b])
        assert idx.ntotal == 40000
        lab, dist = idx.SearchBatch(Q, 50)
        oi, od = io.search(metric, Q, X, 50, ids=ids)
        assert_same(lab, dist, oi, od, "ids")
        # predicate masks: a byte mask (sparse: the row list) and a near-total one (the per-row test)
        for keep in (0.1, 0.5, 0.97):  # (0.5: the MFMA pass over the row list; 0.97: over the per-row test)
            mask = (rng.random(40000) < keep).astype(np.uint8)
            assert idx._lib.lb_gpu_index_set_filter(idx._h, mask.ctypes.data, mask.size) == 0
            vis = np.flatnonzero(mask)
            for nq in (1, 70):
                lab, dist = idx.SearchBatch(Q[:nq], 20)
                if nq == 70 and keep > 0.1:
                    assert idx._lib.lb_gpu_index_last_route(idx._h) == ROUTE_I8_MFMA
                oi, od = io.search(metric, Q[:nq], X, 20, ids=ids, visible=vis)
                assert_same(lab, dist, oi, od, f"mask {keep} nq {nq}")
        col = np.arange(40000) % 7
        assert _filter_int64(idx, col, 3, 0) == 0  # column == 3
        lab, dist = idx.SearchBatch(Q[:5], 10)
        oi, od = io.search(metric, Q[:5], X, 10, ids=ids, visible=np.flatnonzero(col == 3))
        assert_same(lab, dist, oi, od, "filter_int64")
        fcol = (np.arange(40000) % 11).astype(F)
        assert idx._lib.lb_gpu_index_filter_float32(idx._h, fcol.ctypes.data, fcol.size, C.c_float(8.0), 0, None, 0, 0) == 0
        lab, dist = idx.SearchBatch(Q[:5], 10)
        oi, od = io.search(metric, Q[:5], X, 10, ids=ids, visible=np.flatnonzero(fcol == 8.0))
        assert_same(lab, dist, oi, od, "filter_float32")
    finally:
        idx.Close()


def test_device_add_and_search():
    gpu_or_skip()
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(23)
    dim = 768
    X, Q = rows(rng, 30000, dim), rows(rng, 40, dim)  # (40 queries: the MFMA pass reads the caller's device batch)
    idx = new_i8(dim, L2)
    try:
        dX = torch.from_numpy(X).cuda()
        dQ = torch.from_numpy(Q).cuda()
        idx.add_device(X.shape[0], dX.data_ptr())
        dd = torch.empty((40, 10), dtype=torch.float32, device="cuda")
        dl = torch.empty((40, 10), dtype=torch.int64, device="cuda")
        idx.search_device(40, dQ.data_ptr(), 10, dd.data_ptr(), dl.data_ptr())
        torch.cuda.synchronize()
        oi, od = io.search(L2, Q, X, 10)
        assert_same(dl.cpu().numpy(), dd.cpu().numpy(), oi, od, "device")
    finally:
        idx.Close()


def test_hbm_bytes_one_byte_per_element():
    gpu_or_skip()
    from tests.gpu_util import new_index
    n, dim = 100000, 768
    X = np.zeros((n, dim), I8)
    a, b = new_i8(dim, L2), new_index(dim, L2)
    try:
        a.Add(None, X)
        b.set_f16_image(0)
        b.Add(None, X.astype(F))
        ha, hb = a.hbm_bytes(), b.hbm_bytes()
        assert n * dim <= ha < n * dim * 1.25 + (64 << 20), ha
        assert hb - ha >= 3 * n * dim * 0.9, (ha, hb)
    finally:
        a.Close()
        b.Close()


def test_dtype_mismatch_and_unsupported():
    lib = gpu_or_skip()
    from longbow_amd import gpu
    from tests.gpu_util import new_index
    st = C.c_int(0)
    assert not lib.lb_gpu_index_new_i8(0, 16, COS, C.byref(st)) and st.value == 6
    assert not lib.lb_gpu_index_new_i8(0, 4100, DOT, C.byref(st)) and st.value == 6
    assert not lib.lb_gpu_index_new_i8(0, 8193, L2, C.byref(st)) and st.value == 6
    h = lib.lb_gpu_index_new_i8(0, 4096, DOT, C.byref(st))  # floor(4096 / 4) = 1024 chains' terms: accepted
    assert h
    lib.lb_gpu_index_free(h)
    i8 = new_i8(16, L2)
    f32 = new_index(16, L2)
    f16 = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=16, DataType=gpu.DataType.Float16))
    try:
        x8 = np.ones((2, 16), I8)
        xf = np.ones((2, 16), F)
        d = np.empty(2, F)
        lab = np.empty(2, np.int64)
        assert lib.lb_gpu_index_add(i8._h, 2, xf.ctypes.data, None) == 1
        assert lib.lb_gpu_index_add_f16(i8._h, 2, xf.ctypes.data, None) == 1
        assert lib.lb_gpu_index_add_i8(f32._h, 2, x8.ctypes.data, None) == 1
        assert lib.lb_gpu_index_add_i8(f16._h, 2, x8.ctypes.data, None) == 1
        assert b"float32" in lib.lb_gpu_last_error(f32._h)
        i8.Add(None, x8)
        assert lib.lb_gpu_index_search(i8._h, 1, xf.ctypes.data, 1, d.ctypes.data, lab.ctypes.data) == 1
        assert lib.lb_gpu_index_search_f16(i8._h, 1, xf.ctypes.data, 1, d.ctypes.data, lab.ctypes.data) == 1
        assert lib.lb_gpu_index_search_i8(f32._h, 1, x8.ctypes.data, 1, d.ctypes.data, lab.ctypes.data) == 1
        assert lib.lb_gpu_index_search_i8(i8._h, 1, x8.ctypes.data, 1, d.ctypes.data, lab.ctypes.data) == 0
        rows_ = np.zeros(1, np.int64)
        assert lib.lb_gpu_index_rerank(i8._h, xf.ctypes.data, rows_.ctypes.data, 1, 1, d.ctypes.data, None) == 6
        assert lib.lb_gpu_index_dtype(i8._h) == 2
        assert lib.lb_gpu_index_set_candidate_mode(i8._h, 3) == 0  # AUTO
        for mode in (0, 1, 2, 4):
            assert lib.lb_gpu_index_set_candidate_mode(i8._h, mode) == 6
        assert lib.lb_gpu_index_set_f16_image(i8._h, 1) == 0 and lib.lb_gpu_index_f16_image_bytes(i8._h) == 0
        with pytest.raises(TypeError):
            i8.Add(None, xf)
    finally:
        i8.Close()
        f32.Close()
        f16.Close()


def test_comm_refuses_i8_shards():
    lib = gpu_or_skip()
    devs = (C.c_int * 1)(0)
    st = C.c_int(0)
    comm = lib.lb_gpu_comm_init_all(1, devs, C.byref(st))
    assert comm, st.value
    idx = new_i8(16, L2)
    try:
        idx.Add(None, np.ones((4, 16), I8))
        shards = (C.c_void_p * 1)(idx._h)
        q = np.ones((1, 16), F)
        d = np.empty(1, F)
        lab = np.empty(1, np.int64)
        assert lib.lb_gpu_comm_search_all(comm, shards, 1, q.ctypes.data, 1, d.ctypes.data, lab.ctypes.data) == 6
    finally:
        idx.Close()
        lib.lb_gpu_comm_free(comm)


def _ipc(batch):
    import pyarrow as pa
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, batch.schema) as w:
        w.write_batch(batch)
    return sink.getvalue().to_pybytes()


def test_flight_int8_ingest():
    lib = gpu_or_skip()
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(29)
    dim = 32
    X = rows(rng, 3000, dim)
    ids = np.arange(3000, dtype=np.int64) * 3
    vec = pa.FixedSizeListArray.from_arrays(pa.array(X.reshape(-1), pa.int8()), dim)
    batch = pa.record_batch([pa.array(ids, pa.int64()), vec], names=["id", "vector"])
    idx = new_i8(dim, L2)
    try:
        buf = _ipc(batch)
        added = C.c_int64(0)
        err = C.create_string_buffer(256)
        rc = lib.lb_flight_index_add_ipc(idx._h, buf, len(buf), C.byref(added), err, 256)
        assert rc == 0 and added.value == 3000, err.value
        Q = rows(rng, 4, dim)
        lab, dist = idx.SearchBatch(Q, 10)
        oi, od = io.search(L2, Q, X, 10, ids=ids)
        assert_same(lab, dist, oi, od, "ipc")
        # a float32 column is refused on an int8 index
        vf = pa.FixedSizeListArray.from_arrays(pa.array(X.reshape(-1).astype(F), pa.float32()), dim)
        bf = _ipc(pa.record_batch([vf], names=["vector"]))
        assert lib.lb_flight_index_add_ipc(idx._h, bf, len(bf), C.byref(added), err, 256) != 0
        assert b"int8" in err.value
    finally:
        idx.Close()


def test_concurrent_i8_searches_match_serial():
    gpu_or_skip()
    rng = np.random.default_rng(31)
    dim = 256
    X = rows(rng, 60000, dim)
    Q = rows(rng, 96, dim)
    idx = new_i8(dim, DOT)
    try:
        idx.Add(None, X)
        serial = [idx.SearchBatch(Q[i:i + 12], 25) for i in range(0, 96, 12)]
        out = [None] * 8
        errs = []

        def run(t):
            try:
                for _ in range(3):
                    out[t] = idx.SearchBatch(Q[t * 12:(t + 1) * 12], 25)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=run, args=(t,)) for t in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for t in range(8):
            assert np.array_equal(out[t][0], serial[t][0]) and np.array_equal(out[t][1], serial[t][1]), t
        oi, od = io.search(DOT, Q[:12], X, 25)
        assert_same(serial[0][0], serial[0][1], oi, od, "serial")
    finally:
        idx.Close()


def test_1m_x_768_l2_1024_queries():
    gpu_or_skip()
    rng = np.random.default_rng(37)
    n, dim = 1_000_000, 768
    X = rows(rng, n, dim)
    Q = rows(rng, 1024, dim)
    idx = new_i8(dim, L2)
    try:
        idx.Add(None, X)
        lab, dist = idx.SearchBatch(Q, 100)
        assert idx._lib.lb_gpu_index_last_route(idx._h) == ROUTE_I8_MFMA  # (a build that silently scans fails here)
        sample = rng.choice(1024, 32, replace=False)
        oi, od = io.search(L2, Q[sample], X, 100)
        assert_same(lab[sample], dist[sample], oi, od, "1M x 768")
    finally:
        idx.Close()
