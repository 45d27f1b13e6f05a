"""Mirror of store.SQ8Encoder (internal/store/scalar_quantization.go) and an exact k-NN index over its codes by the integer
distance simd.EuclideanDistanceSQ8 (internal/simd/sq8.go), computed by HIP kernels (lb_gpu_sq8_*).

A code is one uint8 per dimension: uint8((clamp(v) - min) * 255 / (max - min)) between per-dimension bounds.  The ranking
distance S = sum (a_i - b_i)^2 is an int32, so codes, distances and labels are exact.  One object is both the encoder and the
index: the codes it stores are searched by position.  A new encoder is untrained: `train` or `set_bounds` gives it its bounds;
what works on codes alone needs none.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._rowfilter import RowFilterMixin

FLT_MAX = np.float32(3.4028234663852886e38)
INT32_MAX = 0x7FFFFFFF


class SQ8Encoder(RowFilterMixin):
    """store.SQ8Encoder on the GPU (untrained until set_bounds / train)."""
    _prefix = "lb_gpu_sq8"

    def __init__(self, dims, device=0, lib=None):
        if dims <= 0:
            raise ValueError(f"dimension must be positive, got {dims}")
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        h = lib.lb_gpu_sq8_new(device, dims, C.byref(st))
        if not h:
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.device = device
        self.Dimensions = dims

    def _check(self, rc):
        _lib.check(rc, self._h, lib=self._lib, prefix=self._prefix)

    def _codes(self, codes):
        c = np.ascontiguousarray(codes, np.uint8)
        single = c.ndim == 1
        c = c.reshape(-1, c.shape[-1]) if c.size else c.reshape(0, self.Dimensions)
        if c.shape[1] != self.Dimensions:
            raise ValueError(f"code length {c.shape[1]} does not match {self.Dimensions} dimensions")
        return c, single

    def _one(self, code):
        q, _ = self._codes(code)
        if q.shape[0] != 1:
            raise ValueError("one query code")
        return q

    def _vectors(self, vectors):
        v = np.ascontiguousarray(vectors, np.float32)
        single = v.ndim == 1
        v = v.reshape(-1, v.shape[-1]) if v.size else v.reshape(0, self.Dimensions)
        if v.shape[1] != self.Dimensions:
            raise ValueError(f"vector dimension {v.shape[1]} does not match {self.Dimensions}")
        return v, single

    # -- bounds ------------------------------------------------------------------
    @property
    def trained(self):
        return bool(self._lib.lb_gpu_sq8_trained(self._h))

    def set_bounds(self, min_vals, max_vals):
        """NewSQ8Encoder (scalar_quantization.go:62-86) on given bounds: Validate refuses min >= max in any dimension"""
        mn = np.ascontiguousarray(min_vals, np.float32).reshape(-1)
        mx = np.ascontiguousarray(max_vals, np.float32).reshape(-1)
        if mn.size != mx.size:
            raise ValueError("min and max must have same length")
        if mn.size != self.Dimensions:
            raise ValueError(f"bounds of length {mn.size} do not match {self.Dimensions} dimensions")
        self._check(self._lib.lb_gpu_sq8_set_bounds(self._h, mn.ctypes.data, mx.ctypes.data))

    def train(self, vectors):
        """TrainSQ8Encoder (scalar_quantization.go:89-134) on f32 rows [n, dims]"""
        v, _ = self._vectors(vectors)
        self._check(self._lib.lb_gpu_sq8_train(self._h, v.shape[0], v.ctypes.data))

    def train_device(self, n, d_vectors):
        self._check(self._lib.lb_gpu_sq8_train_device(self._h, n, d_vectors))

    # -- store.SQ8Encoder --------------------------------------------------------
    def Dims(self):
        """scalar_quantization.go:137-139"""
        return self.Dimensions

    def GetBounds(self):
        """scalar_quantization.go:142-144 -> (min, max)"""
        mn = np.empty(self.Dimensions, np.float32)
        mx = np.empty(self.Dimensions, np.float32)
        self._check(self._lib.lb_gpu_sq8_get_bounds(self._h, mn.ctypes.data, mx.ctypes.data))
        return mn, mx

    def Encode(self, vec):
        """Encode (scalar_quantization.go:147-170): one vector -> dims codes; a 2-D array encodes row by row"""
        v, single = self._vectors(vec)
        codes = np.empty((v.shape[0], self.Dimensions), np.uint8)
        self._check(self._lib.lb_gpu_sq8_encode(self._h, v.shape[0], v.ctypes.data, codes.ctypes.data))
        return codes[0] if single else codes

    def Decode(self, codes):
        """Decode (scalar_quantization.go:173-184)"""
        c, single = self._codes(codes)
        out = np.empty((c.shape[0], self.Dimensions), np.float32)
        self._check(self._lib.lb_gpu_sq8_decode(self._h, c.shape[0], c.ctypes.data, out.ctypes.data))
        return out[0] if single else out

    def _pair(self, q1, q2, want_euclid):
        tmp = SQ8Encoder(self.Dimensions, self.device, lib=self._lib)
        try:
            if want_euclid:
                tmp.set_bounds(*self.GetBounds())
            tmp.add_codes(self._one(q2))
            return tmp.rerank(q1, [0], want_euclid=want_euclid)
        finally:
            tmp.Close()

    def SQ8EuclideanDistance(self, q1, q2):
        """SQ8EuclideanDistance (scalar_quantization.go:192-203) of two codes"""
        return self._pair(q1, q2, True)[1][0]

    def SQ8DistanceFast(self, q1, q2):
        """SQ8DistanceFast (scalar_quantization.go:208-216) of two codes"""
        return int(self._pair(q1, q2, False)[0])

    def distance_batch(self, query, row0=0, n=None):
        """S of one query code against the stored rows [row0, row0 + n) -> int32[n]"""
        q = self._one(query)
        n = self.ntotal - row0 if n is None else n
        out = np.empty(max(n, 0), np.int32)
        self._check(self._lib.lb_gpu_sq8_distance_batch(self._h, q.ctypes.data, row0, n, out.ctypes.data))
        return out

    def EuclideanDistanceSQ8Batch(self, query, candidates=None, row0=0, n=None):
        """simd.EuclideanDistanceSQ8Batch (internal/simd/simd.go:170-182) -> float32(S) [n].  candidates: codes [n, dims]; None:
        the stored rows [row0, row0 + n)."""
        if candidates is not None:
            cand, _ = self._codes(candidates)
            tmp = SQ8Encoder(self.Dimensions, self.device, lib=self._lib)
            try:
                tmp.add_codes(cand)
                return tmp.distance_batch(query).astype(np.float32)
            finally:
                tmp.Close()
        return self.distance_batch(query, row0, n).astype(np.float32)

    # -- the index ---------------------------------------------------------------
    @property
    def ntotal(self):
        return int(self._lib.lb_gpu_sq8_ntotal(self._h))

    def reserve(self, n_total):
        self._check(self._lib.lb_gpu_sq8_reserve(self._h, n_total))

    def add_codes(self, codes):
        """append codes [n, dims] as they are"""
        c, _ = self._codes(codes)
        self._check(self._lib.lb_gpu_sq8_add_codes(self._h, c.shape[0], c.ctypes.data))

    def add_codes_device(self, n, d_codes):
        self._check(self._lib.lb_gpu_sq8_add_codes_device(self._h, n, d_codes))

    def add_vectors(self, vectors):
        """encode f32 rows [n, dims] and append their codes"""
        v, _ = self._vectors(vectors)
        self._check(self._lib.lb_gpu_sq8_add_vectors(self._h, v.shape[0], v.ctypes.data))

    def add_vectors_device(self, n, d_vectors):
        self._check(self._lib.lb_gpu_sq8_add_vectors_device(self._h, n, d_vectors))

    def encode_device(self, n, d_vectors, d_codes, stream=None):
        self._check(self._lib.lb_gpu_sq8_encode_device(self._h, n, d_vectors, d_codes, stream))

    def get_codes(self, row0=0, n=None):
        """stored rows [row0, row0 + n) -> uint8 [n, dims]"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((max(n, 0), self.Dimensions), np.uint8)
        self._check(self._lib.lb_gpu_sq8_get_codes(self._h, row0, n, out.ctypes.data))
        return out

    def rerank(self, qcode, rows, want_euclid=True):
        """S (int32) of the stored rows `rows` to qcode, and SQ8EuclideanDistance of each (a trained encoder); rows outside
        [0, ntotal): INT32_MAX / FLT_MAX"""
        q = self._one(qcode)
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1)
        s = np.empty(rows.size, np.int32)
        e = np.empty(rows.size, np.float32) if want_euclid else None
        self._check(self._lib.lb_gpu_sq8_rerank(self._h, q.ctypes.data, rows.ctypes.data, rows.size, s.ctypes.data,
                                                e.ctypes.data if want_euclid else None))
        return (s, e) if want_euclid else s

    def rerank_device(self, d_qcode, d_rows, n, d_s, d_euclid=None, stream=None):
        self._check(self._lib.lb_gpu_sq8_rerank_device(self._h, d_qcode, d_rows, n, d_s, d_euclid, stream))

    def search_codes(self, qcodes, k):
        """exact k-NN of query codes [nq, dims] -> (labels [nq, k], dist [nq, k] = float32(S)), ascending by (S, position)"""
        q, _ = self._codes(qcodes)
        dist = np.empty((q.shape[0], k), np.float32)
        labels = np.empty((q.shape[0], k), np.int64)
        self._check(self._lib.lb_gpu_sq8_search_codes(self._h, q.shape[0], q.ctypes.data, k, dist.ctypes.data, labels.ctypes.data))
        return labels, dist

    def search(self, queries, k, ctx=None):
        """exact k-NN of f32 queries [nq, dims], encoded on the device first"""
        v, _ = self._vectors(queries)
        dist = np.empty((v.shape[0], k), np.float32)
        labels = np.empty((v.shape[0], k), np.int64)
        self._check(self._lib.lb_gpu_sq8_search_ctx(self._h, v.shape[0], v.ctypes.data, k, dist.ctypes.data, labels.ctypes.data,
                                                    ctx._h if ctx is not None else None))
        return labels, dist

    def search_device(self, nq, d_queries, k, d_dist, d_labels, stream=None, ctx=None):
        self._check(self._lib.lb_gpu_sq8_search_device_ctx(self._h, nq, d_queries, k, d_dist, d_labels, stream,
                                                           ctx._h if ctx is not None else None))

    def search_rerank(self, index, queries, k, oversample):
        return search_rerank(self, index, queries, k, oversample)

    def search_refine(self, index, queries, k, shortlist, order=None):
        """search_rerank's two stages with the second on the device: a shortlist of `shortlist` rows per query by the integer
        distance, then the exact top k of every shortlist on `index` in one call (gpu.Index.Refine; a float32 or float16
        gpu.Index filled in the same row order).  -> (labels [nq, k], dist [nq, k]), padded with -1 / FLT_MAX.  A row filter
        on this handle shapes the shortlist, so the result holds visible rows only; `index` needs no filter."""
        v, _ = self._vectors(queries)
        short, _ = self.search(v, shortlist)
        return index.Refine(v, short, k, order)

    def Close(self):
        if self._h:
            self._lib.lb_gpu_sq8_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


def train(vectors, device=0, lib=None):
    """TrainSQ8Encoder (scalar_quantization.go:89-134): an encoder with the bounds of `vectors` [n, dims]"""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2 or v.shape[0] == 0:
        raise ValueError("no vectors provided for training")
    if v.shape[1] == 0:
        raise ValueError("vectors have zero dimensions")
    enc = SQ8Encoder(v.shape[1], device, lib=lib)
    try:
        enc.train(v)
    except Exception:
        enc.Close()
        raise
    return enc


def search_rerank(sq8, index, queries, k, oversample):
    """The two-stage use the codes exist for: a shortlist of k * oversample rows per query by the integer distance, then the
    exact distances of those rows on `index` (a float32 gpu.Index filled in the same row order; lb_gpu_index_rerank), sorted
    by (distance, position) and cut to k.  -> (labels [nq, k], dist [nq, k]), padded with -1 / FLT_MAX.
    Under a row filter on the encoder (set_filter / filter_column) the shortlist holds visible rows only, and the re-rank
    addresses rows directly, so the result is the filtered one: nothing here changes, and `index` needs no filter."""
    v, _ = sq8._vectors(queries)
    short, _ = sq8.search(v, k * oversample)
    labels = np.full((v.shape[0], k), -1, np.int64)
    dist = np.full((v.shape[0], k), FLT_MAX, np.float32)
    for q in range(v.shape[0]):
        rows = short[q][short[q] >= 0]
        d = index.Rerank(v[q], rows, want_score=False)
        keep = np.lexsort((rows, d))[:k]
        labels[q, :keep.size] = rows[keep]
        dist[q, :keep.size] = d[keep]
    return labels, dist
