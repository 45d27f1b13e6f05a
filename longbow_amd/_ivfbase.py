"""What the IVF handles share on the <_prefix>_* entry points: ivf.IVFFlat (rows) and ivfpq.IVFPQ (codes) over one coarse partition."""
import ctypes as C

import numpy as np

from . import _lib


class IVFBase:
    """A handle with centroids f32 [nlist, dims] given at creation.  A subclass sets _prefix and _timing_slots, and in its __init__
    self._lib, self._h, self.nlist and self.dims (self._h = None first: Close() and __del__ find that when creation fails)."""
    _prefix = None  # "lb_gpu_ivf" / "lb_gpu_ivfpq"
    _timing_slots = 0
    _has_ids = False  # an add gave ids: the searches then return those and not row positions (search_refine needs positions)

    def _fn(self, name):
        return getattr(self._lib, self._prefix + "_" + name)

    def _check(self, rc):
        _lib.check(rc, self._h, lib=self._lib, prefix=self._prefix)

    def _vectors(self, vectors):
        v = np.ascontiguousarray(vectors, np.float32)
        v = v.reshape(-1, v.shape[-1]) if v.size else v.reshape(0, self.dims)
        if v.shape[1] != self.dims:
            raise ValueError(f"vector dimension {v.shape[1]} does not match {self.dims}")
        return v

    @property
    def ntotal(self):
        return int(self._fn("ntotal")(self._h))

    @property
    def hbm_bytes(self):
        return int(self._fn("hbm_bytes")(self._h))

    def centroids(self):
        out = np.empty((self.nlist, self.dims), np.float32)
        self._check(self._fn("get_centroids")(self._h, out.ctypes.data))
        return out

    def reserve(self, n_total):
        self._check(self._fn("reserve")(self._h, n_total))

    def add(self, vectors, ids=None):
        """append rows [n, dims]; ids (int64 [n]) on every add or on none.  Each add rebuilds the lists of all rows: O(ntotal)."""
        self._add(self._vectors(vectors), ids, "add")

    def _add(self, v, ids, entry):
        """rows v [n, dims], contiguous and of the element type that the entry point `entry` takes"""
        i = None
        if ids is not None:
            i = np.ascontiguousarray(ids, np.int64).reshape(-1)
            if i.size != v.shape[0]:
                raise ValueError(f"{i.size} ids for {v.shape[0]} rows")
        self._check(self._fn(entry)(self._h, v.shape[0], v.ctypes.data, i.ctypes.data if i is not None else None))
        self._has_ids = self._has_ids or i is not None

    def add_device(self, n, d_vectors, d_ids=None):
        self._check(self._fn("add_device")(self._h, n, d_vectors, d_ids))
        self._has_ids = self._has_ids or d_ids is not None

    def list_sizes(self):
        out = np.empty(self.nlist, np.int64)
        self._check(self._fn("list_sizes")(self._h, out.ctypes.data))
        return out

    def assignments(self, row0=0, n=None):
        """the lists of rows [row0, row0 + n) -> int32 [n]"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty(max(n, 0), np.int32)
        self._check(self._fn("assignments")(self._h, row0, n, out.ctypes.data))
        return out

    def search(self, queries, k, nprobe, ctx=None):
        """-> (labels [nq, k], dist [nq, k]): ascending (distance, row) among the rows of the probed lists, padded -1 / FLT_MAX"""
        return self._search_host("search", self._vectors(queries), k, nprobe, ctx)

    def search_device(self, nq, d_queries, k, nprobe, d_dist, d_labels, stream=None, ctx=None):
        self._search_dev("search", nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx)

    def _search_host(self, entry, v, k, nprobe, ctx, bitmap=None, bitmap_stride=0):
        """queries v [nq, dims] of the element type that <entry>_ctx takes; bitmap: None, or the LSB-first bits of ntotal row
        positions as uint8 (ivf.pack_bitmap), one bitmap for every query (bitmap_stride 0) or query q's at q * bitmap_stride bytes:
        <entry>_bitmap_ctx, on the handles that have it"""
        dist = np.empty((v.shape[0], k), np.float32)
        labels = np.empty((v.shape[0], k), np.int64)
        c = ctx._h if ctx is not None else None
        if bitmap is None:
            self._check(self._fn(entry + "_ctx")(self._h, v.shape[0], v.ctypes.data, k, nprobe, dist.ctypes.data, labels.ctypes.data, c))
            return labels, dist
        b = np.ascontiguousarray(bitmap, np.uint8).reshape(-1)
        n = self.ntotal
        need = (max(v.shape[0], 1) - 1) * bitmap_stride + (n + 7) // 8 if bitmap_stride > 0 else (n + 7) // 8
        if b.size < need or (bitmap_stride == 0 and b.size != need):  # (the bits of ntotal rows, no more: an old length is caught)
            raise ValueError(f"a bitmap of {b.size} bytes, {need} are read for {n} rows at stride {bitmap_stride}")
        if b.size == 0:
            b = np.zeros(1, np.uint8)  # (an empty handle: a bitmap that is there, and of which nothing is read)
        self._check(self._fn(entry + "_bitmap_ctx")(self._h, v.shape[0], v.ctypes.data, k, nprobe, b.ctypes.data, n, bitmap_stride,
                                                    dist.ctypes.data, labels.ctypes.data, c))
        return labels, dist

    def _search_dev(self, entry, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, d_bitmap=None, nbits=0, bitmap_stride=0):
        c = ctx._h if ctx is not None else None
        if d_bitmap is None:
            self._check(self._fn(entry + "_device_ctx")(self._h, nq, d_queries, k, nprobe, d_dist, d_labels, stream, c))
        else:
            self._check(self._fn(entry + "_bitmap_device_ctx")(self._h, nq, d_queries, k, nprobe, d_bitmap, nbits, bitmap_stride,
                                                               d_dist, d_labels, stream, c))

    def last_search_stats(self):
        """of the last search: (queries, rows scanned summed over them, the largest per-query count, queries selected from LDS)"""
        out = (C.c_int64 * 4)()
        self._check(self._fn("last_search_stats")(self._h, out))
        return tuple(int(x) for x in out)

    def set_profiling(self, on):
        self._check(self._fn("set_profiling")(self._h, 1 if on else 0))

    def last_timing(self):
        """ms of the last profiled search, summed over its batches: _timing_slots values, named by the subclass"""
        out = (C.c_float * self._timing_slots)()
        self._check(self._fn("last_timing")(self._h, out))
        return tuple(float(x) for x in out)

    def Close(self):
        if self._h:
            self._fn("free")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass
