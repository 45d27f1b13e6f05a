"""IVF-PQ on the GPU (lb_gpu_ivfpq_*): the coarse partition of ivf.IVFFlat over the codes of pq.PQEncoder.

A query skips most rows and a row costs M bytes.  Given the codes and the probed lists nothing is approximate: the result is the
exact ADC k-NN among the rows of the probed lists, bit for bit in the reference's BuildADCTable / ADCDistanceBatch arithmetic, and
with every list probed it equals pq.PQEncoder.Search over the same codes.  The codes are plain, not residual: a query's one table
serves every list.  include/longbow_gpu.h states the semantics.

  IVFPQ   the handle: codebooks and centroids given at creation, add / search / codes / list_sizes / assignments / last_search_stats
  train   (centroids, codebook blob) from ivf.train and pq.train
"""
import ctypes as C

import numpy as np

from . import _lib, ivf, pq

FLT_MAX = ivf.FLT_MAX


def train(vectors, nlist, M, max_iter=20, seed=0, device=0):
    """-> (centroids f32 [nlist, dims], codebook blob): ivf.train for the coarse quantiser, pq.train (K = 256) for the codebooks,
    both over the same rows"""
    centroids = ivf.train(vectors, nlist, max_iter, seed, device=device)
    blob, _ = pq.train(vectors, M, 256, max_iter, seed, device=device)
    return centroids, blob


class IVFPQ:
    """lb_gpu_ivfpq: codebooks (the reference's serialised blob, or a pq.PQEncoder whose blob is taken), centroids f32
    [nlist, dims], order 0 SEQ / 1 UNROLL4 of the coarse quantiser (L2)"""

    def __init__(self, codebooks, centroids, order=0, device=0, lib=None):
        self._h = None  # (Close() and __del__ find this when creation fails below)
        buf = bytes(codebooks.blob if isinstance(codebooks, pq.PQEncoder) else codebooks)
        c = np.ascontiguousarray(centroids, np.float32)
        if c.ndim != 2 or c.shape[0] == 0 or c.shape[1] == 0:
            raise ValueError("centroids must be a non-empty [nlist, dims] array")
        if len(buf) >= 12 and int.from_bytes(buf[:4], "little") != c.shape[1]:
            raise ValueError(f"centroids of {c.shape[1]} dimensions, codebooks of {int.from_bytes(buf[:4], 'little')}")
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        h = lib.lb_gpu_ivfpq_new(device, buf, len(buf), order, c.shape[0], c.ctypes.data, C.byref(st))
        if not h:
            if st.value == 1:
                raise ValueError("invalid PQ data")  # persistence.go:39-56 error cases, as pq.PQEncoder
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.device = device
        self.nlist, self.dims = c.shape
        self.m = lib.lb_gpu_ivfpq_m(self._h)
        self.order = order

    def _check(self, rc):
        _lib.check(rc, self._h, lib=self._lib, ivfpq=True)

    def _vectors(self, vectors):
        v = np.ascontiguousarray(vectors, np.float32)
        v = v.reshape(-1, v.shape[-1]) if v.size else v.reshape(0, self.dims)
        if v.shape[1] != self.dims:
            raise ValueError(f"vector dimension {v.shape[1]} does not match {self.dims}")
        return v

    @property
    def ntotal(self):
        return int(self._lib.lb_gpu_ivfpq_ntotal(self._h))

    @property
    def hbm_bytes(self):
        return int(self._lib.lb_gpu_ivfpq_hbm_bytes(self._h))

    def centroids(self):
        out = np.empty((self.nlist, self.dims), np.float32)
        self._check(self._lib.lb_gpu_ivfpq_get_centroids(self._h, out.ctypes.data))
        return out

    def reserve(self, n_total):
        self._check(self._lib.lb_gpu_ivfpq_reserve(self._h, n_total))

    def add(self, vectors, ids=None):
        """assign, encode and append rows [n, dims]; ids (int64 [n]) on every add or on none.  Each add rebuilds the lists and
        the list-major codes of all rows: O(ntotal)."""
        v = self._vectors(vectors)
        i = None
        if ids is not None:
            i = np.ascontiguousarray(ids, np.int64).reshape(-1)
            if i.size != v.shape[0]:
                raise ValueError(f"{i.size} ids for {v.shape[0]} rows")
        self._check(self._lib.lb_gpu_ivfpq_add(self._h, v.shape[0], v.ctypes.data, i.ctypes.data if i is not None else None))

    def add_device(self, n, d_vectors, d_ids=None):
        self._check(self._lib.lb_gpu_ivfpq_add_device(self._h, n, d_vectors, d_ids))

    def codes(self, row0=0, n=None):
        """the codes of rows [row0, row0 + n), insertion order -> uint8 [n, M]"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((max(n, 0), self.m), np.uint8)
        self._check(self._lib.lb_gpu_ivfpq_get_codes(self._h, row0, n, out.ctypes.data))
        return out

    def list_sizes(self):
        out = np.empty(self.nlist, np.int64)
        self._check(self._lib.lb_gpu_ivfpq_list_sizes(self._h, out.ctypes.data))
        return out

    def assignments(self, row0=0, n=None):
        """the lists of rows [row0, row0 + n) -> int32 [n]"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty(max(n, 0), np.int32)
        self._check(self._lib.lb_gpu_ivfpq_assignments(self._h, row0, n, out.ctypes.data))
        return out

    def search(self, queries, k, nprobe, ctx=None):
        """-> (labels [nq, k], dist [nq, k]): ascending (ADC distance, row) among the rows of the probed lists, padded -1 / FLT_MAX"""
        v = self._vectors(queries)
        dist = np.empty((v.shape[0], k), np.float32)
        labels = np.empty((v.shape[0], k), np.int64)
        self._check(self._lib.lb_gpu_ivfpq_search_ctx(self._h, v.shape[0], v.ctypes.data, k, nprobe, dist.ctypes.data, labels.ctypes.data,
                                                      ctx._h if ctx is not None else None))
        return labels, dist

    def search_device(self, nq, d_queries, k, nprobe, d_dist, d_labels, stream=None, ctx=None):
        self._check(self._lib.lb_gpu_ivfpq_search_device_ctx(self._h, nq, d_queries, k, nprobe, d_dist, d_labels, stream,
                                                             ctx._h if ctx is not None else None))

    def last_search_stats(self):
        """of the last search: (queries, rows scanned summed over them, the largest per-query count, queries selected from LDS)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.lb_gpu_ivfpq_last_search_stats(self._h, out))
        return tuple(int(x) for x in out)

    def set_profiling(self, on):
        self._check(self._lib.lb_gpu_ivfpq_set_profiling(self._h, 1 if on else 0))

    def last_timing(self):
        """ms of the last profiled search, summed over its batches: (probes, plan, ADC tables, scan, selection)"""
        out = (C.c_float * 5)()
        self._check(self._lib.lb_gpu_ivfpq_last_timing(self._h, out))
        return tuple(float(x) for x in out)

    def Close(self):
        if self._h:
            self._lib.lb_gpu_ivfpq_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass
