"""Mirror of store.BQEncoder (internal/store/binary_quantization.go) and an exact Hamming k-NN index over its codes, computed
by HIP kernels (lb_gpu_bq_*).

Codes are W = (dims + 63) // 64 little-endian uint64 words per row: bit i % 64 of word i // 64 is set iff v[i] > 0.  Distances
are popcounts of the XOR over whole words (simd.HammingDistance, internal/simd/simd_bitops.go:40-55), so everything is
integer-exact.  One object is both the encoder and the index: the codes it stores are searched by position.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._rowfilter import RowFilterMixin

FLT_MAX = np.float32(3.4028234663852886e38)


class BQEncoder(RowFilterMixin):
    """NewBQEncoder(dims) (binary_quantization.go:16-20) on the GPU."""
    _prefix = "lb_gpu_bq"

    def __init__(self, dims, device=0, lib=None):
        if dims <= 0:
            raise ValueError(f"dimension must be positive, got {dims}")
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        h = lib.lb_gpu_bq_new(device, dims, C.byref(st))
        if not h:
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.device = device
        self.Dimensions = dims
        self.W = lib.lb_gpu_bq_words(self._h)

    def _check(self, rc):
        _lib.check(rc, self._h, lib=self._lib, prefix=self._prefix)

    def _codes(self, codes):
        c = np.ascontiguousarray(codes, np.uint64)
        single = c.ndim == 1
        c = c.reshape(-1, c.shape[-1]) if c.size else c.reshape(0, self.W)
        if c.shape[1] != self.W:
            raise ValueError(f"code length {c.shape[1]} does not match {self.W} words")
        return c, single

    def _vectors(self, vectors):
        v = np.ascontiguousarray(vectors, np.float32)
        single = v.ndim == 1
        v = v.reshape(-1, v.shape[-1]) if v.size else v.reshape(0, self.Dimensions)
        if v.shape[1] != self.Dimensions:
            raise ValueError(f"vector dimension {v.shape[1]} does not match {self.Dimensions}")
        return v, single

    # -- store.BQEncoder ---------------------------------------------------------
    def CodeSize(self):
        """binary_quantization.go:63-65"""
        return self.W

    def Encode(self, vec):
        """Encode (binary_quantization.go:24-48): one vector -> W words; a 2-D array encodes row by row"""
        v, single = self._vectors(vec)
        codes = np.empty((v.shape[0], self.W), np.uint64)
        self._check(self._lib.lb_gpu_bq_encode(self._h, v.shape[0], v.ctypes.data, codes.ctypes.data))
        return codes[0] if single else codes

    def Decode(self, codes):
        """Decode (binary_quantization.go:80-92): bit 1 -> 1.0, bit 0 -> -1.0"""
        c, single = self._codes(codes)
        out = np.empty((c.shape[0], self.Dimensions), np.float32)
        self._check(self._lib.lb_gpu_bq_decode(self._h, c.shape[0], c.ctypes.data, out.ctypes.data))
        return out[0] if single else out

    def HammingDistanceBatch(self, query, candidates=None, row0=0, n=None):
        """HammingDistanceBatch (binary_quantization.go:56-60) -> int32[n].  candidates: codes [n, W]; None: the stored rows
        [row0, row0 + n)."""
        q, _ = self._codes(query)
        if q.shape[0] != 1:
            raise ValueError("one query code")
        if candidates is not None:
            cand, _ = self._codes(candidates)
            tmp = BQEncoder(self.Dimensions, self.device, lib=self._lib)
            try:
                tmp.add_codes(cand)
                return tmp.HammingDistanceBatch(q)
            finally:
                tmp.Close()
        n = self.ntotal - row0 if n is None else n
        out = np.empty(max(n, 0), np.int32)
        self._check(self._lib.lb_gpu_bq_hamming_batch(self._h, q.ctypes.data, row0, n, out.ctypes.data))
        return out

    def HammingDistance(self, a, b):
        """HammingDistance (binary_quantization.go:51-53)"""
        return int(self.HammingDistanceBatch(a, np.ascontiguousarray(b, np.uint64).reshape(1, -1))[0])

    def ScoreToFloat32(self, hamming):
        """binary_quantization.go:69-71, in f32 operations"""
        return np.float32(1.0) - np.float32(hamming) / np.float32(self.Dimensions)

    def Float32ToHamming(self, score):
        """binary_quantization.go:74-76: host arithmetic in float64 on the f32 score"""
        return int(math.floor(float(self.Dimensions) * (1.0 - float(np.float32(score)))))

    # -- the index ---------------------------------------------------------------
    @property
    def ntotal(self):
        return int(self._lib.lb_gpu_bq_ntotal(self._h))

    def reserve(self, n_total):
        self._check(self._lib.lb_gpu_bq_reserve(self._h, n_total))

    def add_codes(self, codes):
        """append codes [n, W] as they are: pad bits a caller sets count in every distance"""
        c, _ = self._codes(codes)
        self._check(self._lib.lb_gpu_bq_add_codes(self._h, c.shape[0], c.ctypes.data))

    def add_codes_device(self, n, d_codes):
        self._check(self._lib.lb_gpu_bq_add_codes_device(self._h, n, d_codes))

    def add_vectors(self, vectors):
        """encode f32 rows [n, dims] and append their codes"""
        v, _ = self._vectors(vectors)
        self._check(self._lib.lb_gpu_bq_add_vectors(self._h, v.shape[0], v.ctypes.data))

    def add_vectors_device(self, n, d_vectors):
        self._check(self._lib.lb_gpu_bq_add_vectors_device(self._h, n, d_vectors))

    def encode_device(self, n, d_vectors, d_codes, stream=None):
        self._check(self._lib.lb_gpu_bq_encode_device(self._h, n, d_vectors, d_codes, stream))

    def get_codes(self, row0=0, n=None):
        """stored rows [row0, row0 + n) -> uint64 [n, W]"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((max(n, 0), self.W), np.uint64)
        self._check(self._lib.lb_gpu_bq_get_codes(self._h, row0, n, out.ctypes.data))
        return out

    def rerank(self, qcode, rows, want_score=True):
        """distances (as f32) of the stored rows `rows` to qcode, and ScoreToFloat32 of each; rows outside [0, ntotal):
        FLT_MAX / 0"""
        q, _ = self._codes(qcode)
        if q.shape[0] != 1:
            raise ValueError("one query code")
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1)
        dist = np.empty(rows.size, np.float32)
        score = np.empty(rows.size, np.float32) if want_score else None
        self._check(self._lib.lb_gpu_bq_rerank(self._h, q.ctypes.data, rows.ctypes.data, rows.size, dist.ctypes.data,
                                               score.ctypes.data if want_score else None))
        return (dist, score) if want_score else dist

    def rerank_device(self, d_qcode, d_rows, n, d_dist, d_score=None, stream=None):
        self._check(self._lib.lb_gpu_bq_rerank_device(self._h, d_qcode, d_rows, n, d_dist, d_score, stream))

    def search_codes(self, qcodes, k):
        """exact k-NN of query codes [nq, W] -> (labels [nq, k], dist [nq, k]), ascending by (distance, position)"""
        q, _ = self._codes(qcodes)
        dist = np.empty((q.shape[0], k), np.float32)
        labels = np.empty((q.shape[0], k), np.int64)
        self._check(self._lib.lb_gpu_bq_search_codes(self._h, q.shape[0], q.ctypes.data, k, dist.ctypes.data, labels.ctypes.data))
        return labels, dist

    def search(self, queries, k, ctx=None):
        """exact k-NN of f32 queries [nq, dims], encoded on the device first"""
        v, _ = self._vectors(queries)
        dist = np.empty((v.shape[0], k), np.float32)
        labels = np.empty((v.shape[0], k), np.int64)
        self._check(self._lib.lb_gpu_bq_search_ctx(self._h, v.shape[0], v.ctypes.data, k, dist.ctypes.data, labels.ctypes.data,
                                                   ctx._h if ctx is not None else None))
        return labels, dist

    def search_device(self, nq, d_queries, k, d_dist, d_labels, stream=None, ctx=None):
        self._check(self._lib.lb_gpu_bq_search_device_ctx(self._h, nq, d_queries, k, d_dist, d_labels, stream,
                                                          ctx._h if ctx is not None else None))

    def search_rerank(self, index, queries, k, oversample):
        return search_rerank(self, index, queries, k, oversample)

    def search_refine(self, index, queries, k, shortlist, order=None):
        """search_rerank's two stages with the second on the device: a Hamming shortlist of `shortlist` rows per query, then the
        exact top k of every shortlist on `index` in one call (gpu.Index.Refine; a float32 or float16 gpu.Index filled in the
        same row order).  -> (labels [nq, k], dist [nq, k]), padded with -1 / FLT_MAX.  A row filter on this handle shapes
        the shortlist, so the result holds visible rows only; `index` needs no filter."""
        v, _ = self._vectors(queries)
        short, _ = self.search(v, shortlist)
        return index.Refine(v, short, k, order)

    def Close(self):
        if self._h:
            self._lib.lb_gpu_bq_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


def search_rerank(bq, index, queries, k, oversample):
    """The two-stage use the codes exist for: a Hamming shortlist of k * oversample rows per query, then the exact distances
    of those rows on `index` (a float32 gpu.Index filled in the same row order; lb_gpu_index_rerank), sorted by
    (distance, position) and cut to k.  -> (labels [nq, k], dist [nq, k]), padded with -1 / FLT_MAX.
    Under a row filter on the encoder (set_filter / filter_column) the shortlist holds visible rows only, and the re-rank
    addresses rows directly, so the result is the filtered one: nothing here changes, and `index` needs no filter."""
    v, _ = bq._vectors(queries)
    short, _ = bq.search(v, k * oversample)
    labels = np.full((v.shape[0], k), -1, np.int64)
    dist = np.full((v.shape[0], k), FLT_MAX, np.float32)
    for q in range(v.shape[0]):
        rows = short[q][short[q] >= 0]
        d = index.Rerank(v[q], rows, want_score=False)
        keep = np.lexsort((rows, d))[:k]
        labels[q, :keep.size] = rows[keep]
        dist[q, :keep.size] = d[keep]
    return labels, dist
