"""float16 index on the device: rows held as IEEE binary16, results bit-identical to the reference's F16 functions, i.e. to the
f32 oracle on the widened data (tests/test_f16_semantics.py pins that premise)."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import oracle_c as oc
from tests.gpu_util import assert_same, gpu_or_skip, oracle_topk_rows_parallel

pytestmark = pytest.mark.gpu

F, H = np.float32, np.float16
L2, COS, DOT = 0, 1, 2


def new_f16(dim, metric, order=None):
    from longbow_amd import gpu
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=dim, Metric=metric, DataType=gpu.DataType.Float16))
    if order is not None:
        idx.set_order(order)
    return idx


def corpus(rng, n, dim):
    return rng.standard_normal((n, dim)).astype(H)


IMAGE_ROUTES = (63, 73)  # fp16 single product (split 3): 256 x 256 tiles (6) or the one 64- / 128-query tile (7), over the image


@pytest.mark.parametrize("metric", [L2, COS, DOT])
@pytest.mark.parametrize("dim", [7, 100, 128, 768])
def test_f16_grid(metric, dim):
    gpu_or_skip()
    rng = np.random.default_rng(dim * 3 + metric)
    n = 20000 if dim == 768 else 30000
    X = rng.random((n, dim), dtype=F).astype(H)  # uniform data
    Q = rng.random((1024, dim), dtype=F).astype(H)
    idx = new_f16(dim, metric)
    Xf = X.astype(F)
    from tests.gpu_util import new_index
    ref = new_index(dim, metric)  # an f32 index over the widened rows: what the image route proves there, it must prove here
    try:
        assert idx.dtype() == 1
        idx.Add(None, X)
        ref.Add(None, Xf)
        assert idx.f16_image_bytes > 0  # from 16,384 rows, as on an f32 index
        for order in (oc.UNROLL4, oc.SEQ):
            idx.set_order(order)
            ref.set_order(order)
            for nq in (1, 3, 5, 64, 200, 1024):
                for k in (1, 10, 100, 1000):
                    if nq * k > 64 * 1000 and k > 10:
                        continue  # (the oracle's share of the run time)
                    lab, dist = idx.SearchBatch(Q[:nq], k)
                    oi, od = oc.search_batch(metric, Q[:nq].astype(F), Xf, k, order=order, nthreads=16)
                    ctx = f"metric {metric} dim {dim} nq {nq} k {k} order {order}"
                    assert_same(lab, dist, oi, od, ctx)
                    route = idx._lib.lb_gpu_index_last_route(idx._h)
                    assert route in (0,) + IMAGE_ROUTES, ctx
                    # batches the image route serves at this size.  (At 7 dimensions a batch whose near-ties the keys cannot
                    # separate makes AUTO back off from the route for a few searches -- here to the exact scan, as designed.)
                    if nq >= 64 and k <= 100 and dim >= 100:
                        assert route in IMAGE_ROUTES, f"{ctx}: route {route}"
                    if route in IMAGE_ROUTES:
                        fb = idx._lib.lb_gpu_index_last_fallbacks(idx._h)
                        if dim >= 100:
                            assert fb == 0, ctx
                        elif fb:  # (7 dimensions of uniform fp16 values: near-ties the keys cannot separate, as over f32 rows)
                            ref.SearchBatch(Q[:nq].astype(F), k)
                            assert fb <= ref._lib.lb_gpu_index_last_fallbacks(ref._h), ctx
    finally:
        idx.Close()
        ref.Close()


def test_default_order_is_unroll4_and_single_search():
    gpu_or_skip()
    rng = np.random.default_rng(1)
    X, q = corpus(rng, 5000, 64), rng.standard_normal(64).astype(H)
    idx = new_f16(64, COS)
    try:
        idx.Add(None, X)
        lab, dist = idx.Search(q, 10)
        oi, od = oc.search_batch(COS, q[None].astype(F), X.astype(F), 10, order=oc.UNROLL4)
        assert_same(lab, dist, oi[0], od[0])
    finally:
        idx.Close()


def test_ids_several_adds_reserve_and_filters():
    gpu_or_skip()
    rng = np.random.default_rng(2)
    dim = 96
    parts = [corpus(rng, m, dim) for m in (7000, 12000, 9000)]
    Q = rng.standard_normal((40, dim)).astype(H)
    for with_ids in (False, True):
        idx = new_f16(dim, L2, oc.UNROLL4)
        try:
            idx.reserve(30000)
            X = np.zeros((0, dim), H)
            ids_all = np.zeros(0, np.int64)
            for p in parts:
                ids = (rng.permutation(10 ** 6)[: len(p)].astype(np.int64) + len(ids_all) * 10 ** 6) if with_ids else None
                idx.Add(ids, p)
                X = np.concatenate([X, p])
                ids_all = np.concatenate([ids_all, ids if with_ids else np.arange(len(ids_all), len(ids_all) + len(p))])
                lab, dist = idx.SearchBatch(Q, 20)
                oi, od = oc.search_batch(L2, Q.astype(F), X.astype(F), 20, order=oc.UNROLL4, ids=ids_all if with_ids else None, nthreads=8)
                assert_same(lab, dist, oi, od, f"ids {with_ids} rows {len(X)}")
            mask = (rng.random(len(X)) < 0.3).astype(np.uint8)
            idx.set_filter(mask)
            lab, dist = idx.SearchBatch(Q, 20)
            oi, od = oc.search_batch(L2, Q.astype(F), X.astype(F), 20, order=oc.UNROLL4, mask=mask,
                                     ids=ids_all if with_ids else None, nthreads=8)
            assert_same(lab, dist, oi, od, "set_filter")
            col = rng.integers(0, 100, len(X)).astype(np.int64)
            idx.FilterInt64(col, 50, 4) if hasattr(idx, "FilterInt64") else _filter_int64(idx, col, 50, 4)
            lab, dist = idx.SearchBatch(Q, 20)
            oi, od = oc.search_batch(L2, Q.astype(F), X.astype(F), 20, order=oc.UNROLL4, mask=(col < 50).astype(np.uint8),
                                     ids=ids_all if with_ids else None, nthreads=8)
            assert_same(lab, dist, oi, od, "filter_int64")
        finally:
            idx.Close()


def _filter_int64(idx, col, value, op):
    col = np.ascontiguousarray(col, np.int64)
    assert idx._lib.lb_gpu_index_filter_int64(idx._h, col.ctypes.data, col.size, value, op, None, 0, 0) == 0


def test_image_off_and_small_index_are_exact():
    gpu_or_skip()
    rng = np.random.default_rng(3)
    X, Q = corpus(rng, 10000, 128), rng.standard_normal((64, 128)).astype(H)
    idx = new_f16(128, DOT)
    try:
        idx.Add(None, X)  # (10k rows: below the image's 16,384)
        lab, dist = idx.SearchBatch(Q, 10)
        oi, od = oc.search_batch(DOT, Q.astype(F), X.astype(F), 10, order=oc.UNROLL4, nthreads=8)
        assert_same(lab, dist, oi, od)
        assert idx._lib.lb_gpu_index_last_route(idx._h) == 0 and idx.f16_image_bytes == 0
    finally:
        idx.Close()
    X = corpus(rng, 30000, 128)
    idx = new_f16(128, DOT)
    try:
        idx.set_f16_image(0)
        idx.Add(None, X)
        lab, dist = idx.SearchBatch(Q, 10)
        oi, od = oc.search_batch(DOT, Q.astype(F), X.astype(F), 10, order=oc.UNROLL4, nthreads=8)
        assert_same(lab, dist, oi, od)
        assert idx._lib.lb_gpu_index_last_route(idx._h) == 0 and idx.f16_image_bytes == 0
    finally:
        idx.Close()


@pytest.mark.parametrize("metric", [L2, COS, DOT])
def test_special_values(metric):
    gpu_or_skip()
    rng = np.random.default_rng(4 + metric)
    dim = 64
    X = corpus(rng, 20000, dim)
    X[5] = np.inf
    X[6, 3] = np.nan
    X[7] = np.float16(6e-6)      # subnormal
    X[8] = np.float16(65504)
    X[9] = np.float16(-65504)
    X[10] = 0                    # zero row: cosine 1.0
    X[11:20] *= np.float16(300)  # far outside the norm range of the rest
    Q = np.concatenate([rng.standard_normal((20, dim)).astype(H), X[[7, 8, 10]]])
    idx = new_f16(dim, metric)
    try:
        idx.Add(None, X)
        lab, dist = idx.SearchBatch(Q, 50)
        oi, od = oc.search_batch(metric, Q.astype(F), X.astype(F), 50, order=oc.UNROLL4, nthreads=8)
        assert_same(lab, dist, oi, od)
    finally:
        idx.Close()


def test_hbm_bytes_per_element():
    gpu_or_skip()
    n, dim = 100000, 768
    X = np.random.default_rng(5).random((20000, dim), dtype=F)  # (the image is kept from 16,384 rows)
    idx = new_f16(dim, COS)
    try:
        idx.reserve(n)
        idx.Add(None, X.astype(H))
        assert idx.f16_image_bytes > 0
        assert idx.hbm_bytes() < 4.1 * n * dim, idx.hbm_bytes()
        idx.set_f16_image(0)
        assert idx.f16_image_bytes == 0
        assert idx.hbm_bytes() < 2.1 * n * dim, idx.hbm_bytes()
    finally:
        idx.Close()
    from tests.gpu_util import new_index
    f = new_index(dim, COS)
    try:
        f.reserve(n)
        f.Add(None, X)
        assert f.f16_image_bytes > 0
        assert f._lib.lb_gpu_index_hbm_bytes(f._h) >= 6 * n * dim
        f.set_f16_image(0)
        assert f._lib.lb_gpu_index_hbm_bytes(f._h) >= 4 * n * dim
    finally:
        f.Close()


def test_dtype_mismatch_and_unsupported():
    gpu_or_skip()
    from tests.gpu_util import new_index
    dim = 32
    h16 = new_f16(dim, L2)
    h32 = new_index(dim, L2)
    try:
        lib = h16._lib
        x32 = np.ones((4, dim), F)
        x16 = np.ones((4, dim), H)
        d = np.empty(4, F)
        lab = np.empty(4, np.int64)
        assert lib.lb_gpu_index_add(h16._h, 4, x32.ctypes.data, None) == 1
        assert b"float16" in lib.lb_gpu_last_error(h16._h)
        assert lib.lb_gpu_index_add_f16(h16._h, 4, x16.ctypes.data, None) == 0
        assert lib.lb_gpu_index_search(h16._h, 1, x32.ctypes.data, 4, d.ctypes.data, lab.ctypes.data) == 1
        assert lib.lb_gpu_index_add_f16(h32._h, 4, x16.ctypes.data, None) == 1
        assert b"float32" in lib.lb_gpu_last_error(h32._h)
        assert lib.lb_gpu_index_search_f16(h32._h, 1, x16.ctypes.data, 4, d.ctypes.data, lab.ctypes.data) == 1
        assert lib.lb_gpu_index_dtype(h32._h) == 0 and lib.lb_gpu_index_dtype(h16._h) == 1
        for mode in (0, 1, 2):
            assert lib.lb_gpu_index_set_candidate_mode(h16._h, mode) == 6
        for mode in (3, 4):
            assert lib.lb_gpu_index_set_candidate_mode(h16._h, mode) == 0
        rows = np.arange(4, dtype=np.int64)
        assert lib.lb_gpu_index_rerank(h16._h, x32.ctypes.data, rows.ctypes.data, 4, -1, d.ctypes.data, None) == 6
        import torch
        dq32 = torch.ones((1, dim), dtype=torch.float32, device="cuda")
        dq16 = torch.ones((1, dim), dtype=torch.float16, device="cuda")
        dd = torch.empty(4, dtype=torch.float32, device="cuda")
        dl = torch.empty(4, dtype=torch.int64, device="cuda")
        drows = torch.arange(4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert lib.lb_gpu_index_rerank_device(h16._h, dq32.data_ptr(), drows.data_ptr(), 4, -1, dd.data_ptr(), None, None) == 6
        assert lib.lb_gpu_index_search_device_ctx(h16._h, 1, dq32.data_ptr(), 4, dd.data_ptr(), dl.data_ptr(), None, None) == 1
        assert lib.lb_gpu_index_search_f16_device_ctx(h32._h, 1, dq16.data_ptr(), 4, dd.data_ptr(), dl.data_ptr(), None, None) == 1
        assert lib.lb_gpu_index_search_f16_device_ctx(h16._h, 1, dq16.data_ptr(), 4, dd.data_ptr(), dl.data_ptr(), None, None) == 0
        torch.cuda.synchronize()
        assert dl.cpu().tolist() == [0, 1, 2, 3]
        with pytest.raises(TypeError):
            h16.Add(None, x32)
    finally:
        h16.Close()
        h32.Close()


def test_comm_refuses_f16_shards():
    lib = gpu_or_skip()
    devs = (C.c_int * 1)(0)
    st = C.c_int(0)
    comm = lib.lb_gpu_comm_init_all(1, devs, C.byref(st))
    assert comm, st.value
    h16 = new_f16(32, L2)
    try:
        shards = (C.c_void_p * 1)(h16._h.value)
        q = np.ones(32, F)
        d = np.empty(1, F)
        lab = np.empty(1, np.int64)
        assert lib.lb_gpu_comm_search_all(comm, shards, 1, q.ctypes.data, 1, d.ctypes.data, lab.ctypes.data) == 6
        import torch
        dq = torch.ones(32, dtype=torch.float32, device="cuda")
        dd = torch.empty(1, dtype=torch.float32, device="cuda")
        dl = torch.empty(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert lib.lb_gpu_comm_search_device(comm, h16._h, 1, dq.data_ptr(), 1, dd.data_ptr(), dl.data_ptr(), None) == 6
    finally:
        h16.Close()
        lib.lb_gpu_comm_free(comm)


def _ipc(batch):
    import pyarrow as pa
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, batch.schema) as w:
        w.write_batch(batch)
    return sink.getvalue().to_pybytes()


def test_flight_halffloat_ingest():
    lib = gpu_or_skip()
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(6)
    dim, n = 48, 3000
    X = corpus(rng, n, dim)
    ids = rng.permutation(10 ** 6)[:n].astype(np.uint64)

    def batch(values, typ):
        col = pa.FixedSizeListArray.from_arrays(pa.array(values.reshape(-1), typ), dim)
        return pa.record_batch([pa.array(ids, pa.uint64()), col], names=["id", "vector"])

    a, b = new_f16(dim, COS), new_f16(dim, COS)
    from tests.gpu_util import new_index
    f = new_index(dim, COS)
    try:
        err = C.create_string_buffer(512)
        added = C.c_int64(0)
        data = _ipc(batch(X, pa.float16()))
        assert lib.lb_flight_index_add_ipc(a._h, data, len(data), C.byref(added), err, 512) == 0, err.value
        assert added.value == n
        b.Add(ids.astype(np.int64), X)
        Q = rng.standard_normal((8, dim)).astype(H)
        la, da = a.SearchBatch(Q, 10)
        lb_, db = b.SearchBatch(Q, 10)
        assert_same(la, da, lb_, db)
        data32 = _ipc(batch(X.astype(F), pa.float32()))
        assert lib.lb_flight_index_add_ipc(a._h, data32, len(data32), C.byref(added), err, 512) == 3  # INVALID_ARGUMENT
        assert lib.lb_flight_index_add_ipc(f._h, data, len(data), C.byref(added), err, 512) == 3
        assert lib.lb_gpu_index_ntotal(a._h) == n
        # the exchange's query column is float32: a dataset backed by a float16 index answers UNIMPLEMENTED (12)
        reg = lib.lb_flight_datasets_new()
        try:
            assert lib.lb_flight_datasets_put(reg, b"half", a._h) == 0
            req = pa.record_batch([pa.array(["half"]), pa.array([10], pa.int32()),
                                   pa.FixedSizeListArray.from_arrays(pa.array(np.ones(dim, F)), dim)], names=["dataset", "k", "query_vector"])
            rb = _ipc(req)
            out = C.c_void_p()
            nout = C.c_size_t(0)
            assert lib.lb_flight_vector_search_exchange(reg, rb, len(rb), C.byref(out), C.byref(nout), err, 512) == 12
        finally:
            lib.lb_flight_datasets_free(reg)
        from longbow_amd import arrow_io, gpu
        ds = arrow_io.GPUDataset("half", dim, metric=COS, data_type=gpu.DataType.Float16)
        try:
            ds.add_ipc_stream(data)
            with pytest.raises(arrow_io.ExchangeError) as e:
                arrow_io.handle_vector_search_exchange({"half": ds}, rb)
            assert "Unimplemented" in str(e.value)
        finally:
            ds.close()
    finally:
        a.Close()
        b.Close()
        f.Close()


def test_concurrent_f16_searches_match_serial():
    gpu_or_skip()
    rng = np.random.default_rng(7)
    dim = 128
    X = corpus(rng, 30000, dim)
    Q = rng.standard_normal((64, dim)).astype(H)
    idx = new_f16(dim, DOT)
    try:
        idx.Add(None, X)
        serial = [idx.Search(Q[i], 10) for i in range(len(Q))]
        out = [None] * len(Q)

        def work(t):
            for i in range(t, len(Q), 8):
                out[i] = idx.Search(Q[i], 10)

        ts = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for i in range(len(Q)):
            assert_same(out[i][0], out[i][1], serial[i][0], serial[i][1], f"query {i}")
    finally:
        idx.Close()


@pytest.mark.parametrize("metric", [COS, DOT])
def test_1m_x_768(metric):
    gpu_or_skip()
    rng = np.random.default_rng(8 + metric)
    n, dim = 1_000_000, 768
    X = rng.standard_normal((n, dim), dtype=F).astype(H)
    Q = rng.standard_normal((1024, dim), dtype=F).astype(H)
    idx = new_f16(dim, metric)
    try:
        idx.Add(None, X)
        lab, dist = idx.SearchBatch(Q, 10)
        Xf = X.astype(F)
        for i in rng.choice(1024, 32, replace=False):
            oi, od = oracle_topk_rows_parallel(oc, metric, Q[i].astype(F), Xf, 10, order=oc.UNROLL4)
            assert_same(lab[i], dist[i], oi, od, f"query {i}")
    finally:
        idx.Close()
