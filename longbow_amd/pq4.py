"""internal/pq at K = 16 on the GPU: 16-centroid codebooks, 4-bit codes and exact ADC k-NN (lb_gpu_pq4_*).

The reference treats small K as a case of its own: Encode's K <= 16 branch (encodeSequential, encoder.go:87-120),
BuildADCTable and ADCDistance at stride K (adc_table.go:46, 77-92).  Across this interface a code row is M bytes, each
below 16, as Encode returns them; in HBM two codes share a byte.
"""
import ctypes as C

import numpy as np

from . import _lib
from .pq import serialize_codebooks, train  # noqa: F401  (the blob layout and the training are pq's)

K = 16


class PQ4Encoder:
    """PQEncoder with K = 16 on the GPU, built from the reference's serialised blob (or trained: PQ4Encoder.Train)."""
    _prefix = "lb_gpu_pq4"

    @classmethod
    def Train(cls, vectors, M, max_iter=20, seed=0, init_rows=None, device=0):
        """NewPQEncoder(dims, M, 16) + Train(vectors): a ready encoder holding the trained codebooks"""
        blob, _ = train(vectors, M, K, max_iter, seed, init_rows, device)
        return cls(blob, device)

    def __init__(self, blob, device=0, lib=None):
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        buf = bytes(blob)
        h = lib.lb_gpu_pq4_new(device, buf, len(buf), C.byref(st))
        if not h:
            if st.value == 1:
                raise ValueError("invalid PQ data")  # persistence.go:39-56 error cases
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.blob = buf
        self.M = lib.lb_gpu_pq4_m(self._h)
        self.Dims = lib.lb_gpu_pq4_dims(self._h)
        self.K = K
        self.SubDim = self.Dims // self.M

    def _check(self, rc):
        _lib.check(rc, self._h, lib=self._lib, prefix=self._prefix)

    def _rows(self, a, dtype, width, what):
        a = np.ascontiguousarray(a, dtype)
        a = a.reshape(-1, a.shape[-1]) if a.ndim else a.reshape(1, 1)
        if a.shape[1] != width:
            raise ValueError(what)
        return a

    def add_codes(self, codes):
        """rows of M bytes, each below 16 (a larger byte: LongbowGPUError, nothing is added)"""
        c = self._rows(codes, np.uint8, self.M, "code length mismatch")
        self._check(self._lib.lb_gpu_pq4_add_codes(self._h, c.shape[0], c.ctypes.data))

    def add_codes_device(self, n, d_codes):
        self._check(self._lib.lb_gpu_pq4_add_codes_device(self._h, n, d_codes))

    def add_vectors(self, vectors):
        """encode the vectors and append their codes"""
        v = self._rows(vectors, np.float32, self.Dims, "vector dimension mismatch")
        self._check(self._lib.lb_gpu_pq4_add_vectors(self._h, v.shape[0], v.ctypes.data))

    def add_vectors_device(self, n, d_vectors):
        self._check(self._lib.lb_gpu_pq4_add_vectors_device(self._h, n, d_vectors))

    @property
    def ntotal(self):
        return int(self._lib.lb_gpu_pq4_ntotal(self._h))

    @property
    def hbm_bytes(self):
        """the rows allocated at ceil(M / 2) bytes each, plus the codebooks"""
        return int(self._lib.lb_gpu_pq4_hbm_bytes(self._h))

    def reserve(self, n_total):
        self._check(self._lib.lb_gpu_pq4_reserve(self._h, n_total))

    def get_codes(self, row0=0, n=None):
        """stored codes rows [row0, row0+n) -> uint8 [n, M], one code a byte"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((n, self.M), np.uint8)
        self._check(self._lib.lb_gpu_pq4_get_codes(self._h, row0, n, out.ctypes.data))
        return out

    def Encode(self, vector):
        """PQEncoder.Encode, K <= 16 branch (encoder.go:87-120): one vector -> M bytes; a 2-D array encodes row by row."""
        single = np.ndim(vector) == 1
        v = self._rows(vector, np.float32, self.Dims, "vector dimension mismatch")  # encoder.go:77-79
        codes = np.empty((v.shape[0], self.M), np.uint8)
        self._check(self._lib.lb_gpu_pq4_encode(self._h, v.shape[0], v.ctypes.data, codes.ctypes.data))
        return codes[0] if single else codes

    def encode_device(self, n, d_vectors, d_codes, stream=None):
        self._check(self._lib.lb_gpu_pq4_encode_device(self._h, n, d_vectors, d_codes, stream))

    def BuildADCTable(self, query):
        query = np.ascontiguousarray(query, np.float32).reshape(-1)
        if query.size != self.Dims:
            raise ValueError("query dimension mismatch")  # adc_table.go:16-18
        table = np.empty(self.M * K, np.float32)
        self._check(self._lib.lb_gpu_pq4_build_adc_table(self._h, query.ctypes.data, table.ctypes.data))
        return table

    def ADCDistanceBatch(self, table, results, row0=0):
        """distances of stored codes [row0, row0+len(results)) -> results"""
        if results.size == 0:
            return
        table = np.ascontiguousarray(table, np.float32)
        if table.size != self.M * K:
            raise ValueError("invalid table size")  # adc_table.go:64-66
        self._check(self._lib.lb_gpu_pq4_adc_distance_batch(self._h, table.ctypes.data, row0, results.size, results.ctypes.data))

    def Search(self, queries, k, ctx=None):
        """-> (labels [nq, k], dist [nq, k]): ascending (distance, row), padded with -1 / FLT_MAX"""
        queries = self._rows(queries, np.float32, self.Dims, "query dimension mismatch")
        nq = queries.shape[0]
        dist = np.empty((nq, k), np.float32)
        labels = np.empty((nq, k), np.int64)
        self._check(self._lib.lb_gpu_pq4_search_ctx(self._h, nq, queries.ctypes.data, k, dist.ctypes.data, labels.ctypes.data,
                                                    ctx._h if ctx is not None else None))
        return labels, dist

    def search_device(self, nq, d_queries, k, d_dist, d_labels, stream=None, ctx=None):
        self._check(self._lib.lb_gpu_pq4_search_device_ctx(self._h, nq, d_queries, k, d_dist, d_labels, stream,
                                                           ctx._h if ctx is not None else None))

    def Close(self):
        if self._h:
            self._lib.lb_gpu_pq4_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass
