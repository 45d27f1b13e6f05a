"""Mirror of internal/pq's query-side interface (the ADC path), computed by HIP kernels.

PQEncoder.{BuildADCTable, ADCDistanceBatch, Serialize/Deserialize blob}
(internal/pq/adc_table.go:15-72, persistence.go:9-73), Encode / Decode (encoder.go:76-158) and Train
(encoder.go:38-73: TrainKMeans per subspace, kmeans.go:64-151; the unseeded draws of the reference are
restated as the counter-based ones include/longbow_gpu.h documents).
"""
import ctypes as C
import struct

import numpy as np

from . import _lib
from ._rowfilter import RowFilterMixin


def serialize_codebooks(codebooks):
    """PQEncoder.Serialize layout (persistence.go:9-35): u32 LE dims, M, K + M*K*SubDim f32 LE."""
    cb = np.ascontiguousarray(codebooks, np.float32)
    M, K, sub = cb.shape
    return struct.pack("<III", M * sub, M, K) + cb.astype("<f4").tobytes()


def _train_args(dims, M, K, n, init_rows):
    size = 12 + M * K * (dims // M) * 4 if M > 0 and K >= 0 and dims > 0 else 12
    blob = np.zeros(size, np.uint8)
    iters = np.zeros(max(M, 1), np.int32)
    rows = None
    if init_rows is not None:
        rows = np.ascontiguousarray(init_rows, np.int64).reshape(-1)
        if rows.size != M * K:
            raise ValueError("init_rows must hold M*K rows")
    return blob, iters, rows


def train(vectors, M, K=256, max_iter=20, seed=0, init_rows=None, device=0, ctx=None):
    """pq.(*PQEncoder).Train (encoder.go:38-73) on the GPU: exact Lloyd k-means per subspace (lb_gpu_pq_train).
    vectors [n, dims] f32; init_rows [M, K] rows whose copies are the first centroids (None: drawn from seed).
    Returns (blob, iters): the persistence.go blob and the iterations each subspace ran."""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2 or v.shape[0] == 0:
        raise ValueError("empty training data")  # encoder.go:40-42
    n, dims = v.shape
    lib = _lib.require_gpu(device)
    blob, iters, rows = _train_args(dims, M, K, n, init_rows)
    _lib.check(lib.lb_gpu_pq_train(device, dims, M, K, n, v.ctypes.data, max_iter, seed, rows.ctypes.data if rows is not None else None,
                                   blob.ctypes.data, blob.size, iters.ctypes.data, ctx._h if ctx is not None else None))
    return blob.tobytes(), iters[:M]


def train_device(n, d_vectors, dims, M, K=256, max_iter=20, seed=0, init_rows=None, device=0, stream=None, ctx=None):
    """train() over n rows already resident on the device (d_vectors: device address); init_rows stays a host array"""
    lib = _lib.require_gpu(device)
    blob, iters, rows = _train_args(dims, M, K, n, init_rows)
    _lib.check(lib.lb_gpu_pq_train_device(device, dims, M, K, n, d_vectors, max_iter, seed, rows.ctypes.data if rows is not None else None,
                                          blob.ctypes.data, blob.size, iters.ctypes.data, stream, ctx._h if ctx is not None else None))
    return blob.tobytes(), iters[:M]


class PQEncoder(RowFilterMixin):
    """PQEncoder on the GPU, built from the reference's serialised blob (or trained: PQEncoder.Train).  set_filter /
    filter_column / nvisible (RowFilterMixin): with a row filter Search returns the exact ADC k-NN among the visible rows."""
    _prefix = "lb_gpu_pq"

    @classmethod
    def Train(cls, vectors, M, max_iter=20, seed=0, init_rows=None, device=0):
        """NewPQEncoder(dims, M, 256) + Train(vectors): a ready encoder holding the trained codebooks"""
        blob, _ = train(vectors, M, 256, max_iter, seed, init_rows, device)
        return cls(blob, device)

    def __init__(self, blob, device=0, lib=None):
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        buf = bytes(blob)
        h = lib.lb_gpu_pq_new(device, buf, len(buf), C.byref(st))
        if not h:
            if st.value == 1:
                raise ValueError("invalid PQ data")  # persistence.go:39-56 error cases
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.blob = buf  # the codebooks as given (ivfpq.IVFPQ takes an encoder for its codebooks)
        self.M = lib.lb_gpu_pq_m(self._h)
        self.Dims = lib.lb_gpu_pq_dims(self._h)
        self.K = 256
        self.SubDim = self.Dims // self.M

    def _check(self, rc):
        _lib.check(rc, self._h, lib=self._lib, prefix=self._prefix)

    def add_codes(self, codes):
        codes = np.ascontiguousarray(codes, np.uint8).reshape(-1)
        if codes.size % self.M:
            raise ValueError("code length mismatch")
        self._check(self._lib.lb_gpu_pq_add_codes(self._h, codes.size // self.M, codes.ctypes.data))

    def add_codes_device(self, n, d_codes):
        self._check(self._lib.lb_gpu_pq_add_codes_device(self._h, n, d_codes))

    @property
    def ntotal(self):
        return int(self._lib.lb_gpu_pq_ntotal(self._h))

    def reserve(self, n_total):
        self._check(self._lib.lb_gpu_pq_reserve(self._h, n_total))

    def get_codes(self, row0=0, n=None):
        """stored codes rows [row0, row0+n) -> uint8 [n, M]"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((n, self.M), np.uint8)
        self._check(self._lib.lb_gpu_pq_get_codes(self._h, row0, n, out.ctypes.data))
        return out

    def Encode(self, vector):
        """PQEncoder.Encode (encoder.go:76-89): one vector -> M bytes; a 2-D array encodes row by row."""
        v = np.ascontiguousarray(vector, np.float32)
        single = v.ndim == 1
        v = v.reshape(-1, v.shape[-1])
        if v.shape[1] != self.Dims:
            raise ValueError("vector dimension mismatch")  # encoder.go:77-79
        codes = np.empty((v.shape[0], self.M), np.uint8)
        self._check(self._lib.lb_gpu_pq_encode(self._h, v.shape[0], v.ctypes.data, codes.ctypes.data))
        return codes[0] if single else codes

    def Decode(self, codes):
        """PQEncoder.Decode (encoder.go:139-158)"""
        c = np.ascontiguousarray(codes, np.uint8)
        single = c.ndim == 1
        c = c.reshape(-1, c.shape[-1])
        if c.shape[1] != self.M:
            raise ValueError("code length mismatch")  # encoder.go:140-142
        out = np.empty((c.shape[0], self.Dims), np.float32)
        self._check(self._lib.lb_gpu_pq_decode(self._h, c.shape[0], c.ctypes.data, out.ctypes.data))
        return out[0] if single else out

    def encode_device(self, n, d_vectors, d_codes, stream=None):
        self._check(self._lib.lb_gpu_pq_encode_device(self._h, n, d_vectors, d_codes, stream))

    def add_vectors_device(self, n, d_vectors):
        """encode n device-resident vectors and append their codes"""
        self._check(self._lib.lb_gpu_pq_add_vectors_device(self._h, n, d_vectors))

    def Rerank(self, query, rows):
        """processChunkInternal's PQ branch (parallel_search.go:292-345): ADC distance of the stored code rows
        + Score = 1/(1+d)"""
        query = np.ascontiguousarray(query, np.float32).reshape(-1)
        if query.size != self.Dims:
            raise ValueError("query dimension mismatch")
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1)
        dist = np.empty(rows.size, np.float32)
        score = np.empty(rows.size, np.float32)
        self._check(self._lib.lb_gpu_pq_rerank(self._h, query.ctypes.data, rows.ctypes.data, rows.size, dist.ctypes.data,
                                               score.ctypes.data))
        return dist, score

    def BuildADCTable(self, query):
        query = np.ascontiguousarray(query, np.float32).reshape(-1)
        if query.size != self.Dims:
            raise ValueError("query dimension mismatch")  # adc_table.go:16-18
        table = np.empty(self.M * self.K, np.float32)
        self._check(self._lib.lb_gpu_pq_build_adc_table(self._h, query.ctypes.data, table.ctypes.data))
        return table

    def ADCDistanceBatch(self, table, results, row0=0):
        """distances of stored codes [row0, row0+len(results)) -> results (adc_table.go:57-72)"""
        if results.size == 0:
            return
        table = np.ascontiguousarray(table, np.float32)
        if table.size != self.M * self.K:
            raise ValueError("invalid table size")  # adc_table.go:64-66
        if row0 + results.size > self.ntotal:
            raise ValueError("flatCodes buffer too small")  # adc_table.go:61-63
        self._check(self._lib.lb_gpu_pq_adc_distance_batch(self._h, table.ctypes.data, row0, results.size,
                                                            results.ctypes.data))

    def set_prefilter(self, on):
        """True (default): byte-table prefilter + exact survivors; False: exact f32-table pass only.  Same results."""
        self._check(self._lib.lb_gpu_pq_set_prefilter(self._h, 1 if on else 0))

    @property
    def last_search_stats(self):
        """what served the last completed device batch, in queries (a refused or failed search leaves the record):
        (planned with a sampled threshold, four-query passes, two-query passes, single prefilter passes,
        redone on the bootstrap schedule, redone on the schedule that cannot overflow)"""
        out = (C.c_int64 * 6)()
        self._check(self._lib.lb_gpu_pq_last_search_stats(self._h, out))
        return tuple(int(v) for v in out)

    def set_search_combining(self, enable):
        """1 (default): concurrent Search calls of a few queries each are answered by one batch (pairs of queries share a pass
        over the codes); 0: every call on its own.  Same results."""
        self._check(self._lib.lb_gpu_pq_set_search_combining(self._h, 1 if enable else 0))

    @property
    def combining_stats(self):
        """(combined batches run, requests they answered)"""
        import ctypes as C
        out = (C.c_int64 * 2)()
        self._check(self._lib.lb_gpu_pq_combining_stats(self._h, out))
        return int(out[0]), int(out[1])

    def Search(self, queries, k, ctx=None):
        queries = np.ascontiguousarray(queries, np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        if queries.shape[1] != self.Dims:
            raise ValueError("query dimension mismatch")
        nq = queries.shape[0]
        dist = np.empty((nq, k), np.float32)
        labels = np.empty((nq, k), np.int64)
        self._check(self._lib.lb_gpu_pq_search_ctx(self._h, nq, queries.ctypes.data, k, dist.ctypes.data,
                                                   labels.ctypes.data, ctx._h if ctx is not None else None))
        return labels, dist

    def search_device(self, nq, d_queries, k, d_dist, d_labels, stream=None, ctx=None):
        self._check(self._lib.lb_gpu_pq_search_device_ctx(self._h, nq, d_queries, k, d_dist, d_labels, stream,
                                                          ctx._h if ctx is not None else None))

    def search_refine(self, index, queries, k, shortlist, order=None):
        """The two-stage use the codes exist for, on the device: the ADC k-NN of `shortlist` rows per query, then the exact top
        k of every shortlist on `index` in one call (gpu.Index.Refine; a float32 or float16 gpu.Index filled in the same row
        order).  -> (labels [nq, k], dist [nq, k]), padded with -1 / FLT_MAX.  A row filter on this handle shapes the
        shortlist, so the result holds visible rows only; `index` needs no filter."""
        short, _ = self.Search(queries, shortlist)
        return index.Refine(np.ascontiguousarray(queries, np.float32).reshape(short.shape[0], -1), short, k, order)

    def set_profiling(self, on):
        self._check(self._lib.lb_gpu_pq_set_profiling(self._h, 1 if on else 0))

    def last_timing(self):
        """(ms of the last query's pass over the codes, ms of the whole search on the device)"""
        ms = (C.c_float * 2)()
        self._check(self._lib.lb_gpu_pq_last_timing(self._h, ms))
        return float(ms[0]), float(ms[1])

    def Close(self):
        if self._h:
            self._lib.lb_gpu_pq_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass
