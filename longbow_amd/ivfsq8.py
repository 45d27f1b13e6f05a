"""IVF-SQ8 on the GPU (lb_gpu_ivfsq8_*): the coarse partition of ivf.IVFFlat over the codes of sq8.SQ8Encoder.

A query skips most rows and a row costs one byte a dimension.  Given the codes and the probed lists nothing is approximate: the
result is the exact k-NN among the rows of the probed lists by the integer distance S = sum (a_i - b_i)^2, in ascending (S, row)
order of the integers and reported as float32(S), and with every list probed it equals sq8.SQ8Encoder.search over the same codes.
include/longbow_gpu.h states the semantics.

  IVFSQ8  the handle: bounds and centroids given at creation, add / search / codes / bounds / list_sizes / assignments /
          last_search_stats, the row filter (set_filter / filter_column / nvisible), removal (remove / remove_rows /
          remove_device / nlive / ndeleted) and compact().  search(..., bitmap=) and search_device(..., d_bitmap=) take a row
          filter of that call alone, which leaves the handle as it is
  pack_bitmap  a byte or bool mask [n] or [nq, n] -> the LSB-first bits such a call takes, and their stride
  train   (centroids, min, max) from ivf.train and sq8.train
"""
import ctypes as C

import numpy as np

from . import _lib, ivf, sq8
from ._ivfbase import IVFBase
from ._rowfilter import RowFilterMixin, pack_bitmap  # noqa: F401  (pack_bitmap: exported here as ivfsq8.pack_bitmap)

FLT_MAX = ivf.FLT_MAX


def train(vectors, nlist, max_iter=20, seed=0, device=0, centroids=None):
    """-> (centroids f32 [nlist, dims], min f32 [dims], max f32 [dims]): ivf.train for the coarse quantiser, sq8.train
    (TrainSQ8Encoder) for the bounds, both over the same rows.  centroids [nlist, dims] (say from ivf.train_coarse, which goes
    past 256 lists) are used as given in place of the coarse step."""
    if centroids is None:
        centroids = ivf.train(vectors, nlist, max_iter, seed, device=device)
    else:
        centroids = ivf.check_centroids(centroids, nlist, np.shape(vectors)[-1])
    enc = sq8.train(vectors, device=device)
    try:
        mn, mx = enc.GetBounds()
    finally:
        enc.Close()
    return centroids, mn, mx


class IVFSQ8(ivf.RemovalMixin, RowFilterMixin, IVFBase):
    """lb_gpu_ivfsq8: SQ8 bounds min / max f32 [dims] (min < max in every dimension, as SQ8Config.Validate asks; NaN bounds pass),
    centroids f32 [nlist, dims], order 0 SEQ / 1 UNROLL4 of the coarse quantiser (L2).  Under a row filter (RowFilterMixin) the
    probes stay as they are and a search sees the visible rows of the probed lists alone."""
    _prefix = "lb_gpu_ivfsq8"
    _timing_slots = 5

    def __init__(self, min, max, centroids, order=0, device=0, lib=None):
        self._h = None  # (Close() and __del__ find this when creation fails below)
        c = np.ascontiguousarray(centroids, np.float32)
        if c.ndim != 2 or c.shape[0] == 0 or c.shape[1] == 0:
            raise ValueError("centroids must be a non-empty [nlist, dims] array")
        mn = np.ascontiguousarray(min, np.float32).reshape(-1)
        mx = np.ascontiguousarray(max, np.float32).reshape(-1)
        if mn.size != mx.size:
            raise ValueError("min and max must have same length")
        if mn.size != c.shape[1]:
            raise ValueError(f"bounds of length {mn.size} do not match centroids of {c.shape[1]} dimensions")
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        h = lib.lb_gpu_ivfsq8_new(device, c.shape[1], mn.ctypes.data, mx.ctypes.data, order, c.shape[0], c.ctypes.data, C.byref(st))
        if not h:
            with np.errstate(invalid="ignore"):
                if st.value == 1 and (mn >= mx).any():
                    raise ValueError("min must be less than max for all dimensions")  # SQ8Config.Validate
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.device = device
        self.nlist, self.dims = c.shape
        self.order = order

    def add(self, vectors, ids=None):
        """assign, encode and append rows [n, dims]; ids (int64 [n]) on every add or on none.  Each add rebuilds the lists of all
        rows: O(ntotal)."""
        super().add(vectors, ids)

    def codes(self, row0=0, n=None):
        """the codes of rows [row0, row0 + n), insertion order -> uint8 [n, dims]"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((max(n, 0), self.dims), np.uint8)
        self._check(self._lib.lb_gpu_ivfsq8_get_codes(self._h, row0, n, out.ctypes.data))
        return out

    def bounds(self):
        """-> (min, max) f32 [dims] each, as given at creation"""
        mn = np.empty(self.dims, np.float32)
        mx = np.empty(self.dims, np.float32)
        self._check(self._lib.lb_gpu_ivfsq8_get_bounds(self._h, mn.ctypes.data, mx.ctypes.data))
        return mn, mx

    def search(self, queries, k, nprobe, ctx=None, bitmap=None, bitmap_stride=0):
        """-> (labels [nq, k], dist [nq, k] = float32(S)): ascending (S, row) of the integers among the rows of the probed lists,
        padded -1 / FLT_MAX.  bitmap: a row filter of this call alone (lb_gpu_ivfsq8_search_bitmap_ctx), the LSB-first bits of
        pack_bitmap over the ntotal row positions; bitmap_stride 0: one bitmap for every query, else query q's bits start at byte
        q * bitmap_stride.  The handle, its own filter and nvisible() stay as they are; searches with different bitmaps may run
        concurrently."""
        return self._search_host("search", self._vectors(queries), k, nprobe, ctx, bitmap, bitmap_stride)

    def search_device(self, nq, d_queries, k, nprobe, d_dist, d_labels, stream=None, ctx=None, d_bitmap=None, nbits=0, bitmap_stride=0):
        """d_bitmap: the call's bitmap in device memory, of nbits == ntotal bits (any byte address)"""
        self._search_dev("search", nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, d_bitmap, nbits, bitmap_stride)

    def search_refine(self, index, queries, k, shortlist, nprobe, order=None, bitmap=None, bitmap_stride=0):
        """The two-stage use the codes exist for, composed as ivfpq.IVFPQ.search_refine: the integer k-NN of `shortlist` rows per
        query among the probed lists, then the exact top k of every shortlist on `index` in one call (gpu.Index.Refine; a
        float32 or float16 gpu.Index filled in the same row order).  -> (labels [nq, k], dist [nq, k]), padded with -1 /
        FLT_MAX.  The shortlist must hold row positions: a handle that was given ids raises ValueError.  A row filter on this
        handle shapes the shortlist, so the result holds visible rows only; `index` needs no filter.  bitmap, bitmap_stride: a
        row filter of this call alone, as search takes it; it goes to the shortlist search, so the refined result holds rows
        with a set bit only.
        Removed rows never enter the shortlist (it holds live rows only), and `index` treats a position it has removed itself as outside the index.  After compact()
        the positions of this handle are the survivors' new ones: `index` must be compacted over the same removals
        (gpu.Index.Compact is stable too), or the positions no longer correspond."""
        if self._has_ids:
            raise ValueError("search_refine needs row positions: this handle was given ids, which its searches return instead")
        v = self._vectors(queries)
        short, _ = self.search(v, shortlist, nprobe, bitmap=bitmap, bitmap_stride=bitmap_stride)
        return index.Refine(v, short, k, order)

    def last_timing(self):
        """ms of the last profiled search, summed over its batches: (probes, plan, the queries' codes, scan, selection).  The
        compaction of the lists under a call's bitmap falls into the plan's."""
        return super().last_timing()

    def last_build_timing(self):
        """ms of the last profiled build of the visible lists (a filter call or an add under a filter): its launches alone"""
        out = C.c_float(0)
        self._check(self._lib.lb_gpu_ivfsq8_last_build_timing(self._h, C.byref(out)))
        return float(out.value)
