"""IVF-BQ on the GPU (lb_gpu_ivfbq_*): the coarse partition of ivf.IVFFlat over the sign-bit codes of bq.BQEncoder.

A query skips most rows and a row costs one bit a dimension.  Given the codes and the probed lists nothing is approximate: the
result is the exact k-NN among the rows of the probed lists by the Hamming distance h = sum popcount(a ^ b), in ascending
(h, row) order and reported as float32(h), and with every list probed it equals bq.BQEncoder.search over the same codes.
include/longbow_gpu.h states the semantics.

  IVFBQ   the handle: centroids given at creation, add / search / codes / list_sizes / assignments / last_search_stats, and the
          row filter (set_filter / filter_column / nvisible)
  train   ivf.train: the centroids are all the training there is
"""
import ctypes as C

import numpy as np

from . import _lib, ivf
from ._ivfbase import IVFBase
from ._rowfilter import RowFilterMixin

FLT_MAX = ivf.FLT_MAX

train = ivf.train


class IVFBQ(RowFilterMixin, IVFBase):
    """lb_gpu_ivfbq: centroids f32 [nlist, dims], order 0 SEQ / 1 UNROLL4 of the coarse quantiser (L2).  Under a row filter
    (RowFilterMixin) the probes stay as they are and a search sees the visible rows of the probed lists alone."""
    _prefix = "lb_gpu_ivfbq"
    _timing_slots = 5

    def __init__(self, centroids, order=0, device=0, lib=None):
        self._h = None  # (Close() and __del__ find this when creation fails below)
        c = np.ascontiguousarray(centroids, np.float32)
        if c.ndim != 2 or c.shape[0] == 0 or c.shape[1] == 0:
            raise ValueError("centroids must be a non-empty [nlist, dims] array")
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        h = lib.lb_gpu_ivfbq_new(device, c.shape[1], order, c.shape[0], c.ctypes.data, C.byref(st))
        if not h:
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.device = device
        self.nlist, self.dims = c.shape
        self.order = order

    @property
    def words(self):
        """W = (dims + 63) // 64 uint64 words of a code"""
        return int(self._lib.lb_gpu_ivfbq_words(self._h))

    def add(self, vectors, ids=None):
        """assign, encode and append rows [n, dims]; ids (int64 [n]) on every add or on none.  Each add rebuilds the lists of all
        rows and the list-major copy of their codes: O(ntotal)."""
        super().add(vectors, ids)

    def codes(self, row0=0, n=None):
        """the codes of rows [row0, row0 + n), insertion order -> uint64 [n, W]"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((max(n, 0), self.words), np.uint64)
        self._check(self._lib.lb_gpu_ivfbq_get_codes(self._h, row0, n, out.ctypes.data))
        return out

    def search(self, queries, k, nprobe, ctx=None):
        """-> (labels [nq, k], dist [nq, k] = float32(h)): ascending (h, row) among the rows of the probed lists, padded
        -1 / FLT_MAX"""
        return super().search(queries, k, nprobe, ctx)

    def search_refine(self, index, queries, k, shortlist, nprobe, order=None):
        """The two-stage use the codes exist for, composed as ivfsq8.IVFSQ8.search_refine: the Hamming k-NN of `shortlist` rows per
        query among the probed lists, then the exact top k of every shortlist on `index` in one call (gpu.Index.Refine; a
        float32 or float16 gpu.Index filled in the same row order).  -> (labels [nq, k], dist [nq, k]), padded with -1 /
        FLT_MAX.  The shortlist must hold row positions: a handle that was given ids raises ValueError.  A row filter on this
        handle shapes the shortlist, so the result holds visible rows only; `index` needs no filter."""
        if self._has_ids:
            raise ValueError("search_refine needs row positions: this handle was given ids, which its searches return instead")
        v = self._vectors(queries)
        short, _ = self.search(v, shortlist, nprobe)
        return index.Refine(v, short, k, order)

    def last_timing(self):
        """ms of the last profiled search, summed over its batches: (probes, plan, the queries' codes, scan, selection)"""
        return super().last_timing()

    def last_build_timing(self):
        """ms of the last profiled build of the visible lists (a filter call or an add under a filter): its launches alone"""
        out = C.c_float(0)
        self._check(self._lib.lb_gpu_ivfbq_last_build_timing(self._h, C.byref(out)))
        return float(out.value)
