"""IVF-PQ on the GPU (lb_gpu_ivfpq_*): the coarse partition of ivf.IVFFlat over the codes of pq.PQEncoder.

A query skips most rows and a row costs M bytes.  Given the codes and the probed lists nothing is approximate: the result is the
exact ADC k-NN among the rows of the probed lists, bit for bit in the reference's BuildADCTable / ADCDistanceBatch arithmetic, and
with every list probed a plain handle equals pq.PQEncoder.Search over the same codes.

A handle holds one of two kinds of codes, fixed at creation.  Plain (the default): a row is encoded as it is and a query's one
table serves every list.  Residual (residual=True): a row is encoded as its f32 difference from its list's centroid, so the
codebooks spend their words on the spread inside a list; a query then has a table per probed list, built from q - C[l], and the
result is as exact over those tables.  include/longbow_gpu.h states the semantics of both.

  IVFPQ   the handle: codebooks and centroids given at creation, add / search / codes / list_sizes / assignments / last_search_stats,
          the row filter (set_filter / filter_column / nvisible), removal (remove / remove_rows / remove_device / nlive /
          ndeleted) and compact(): codes are kept until compaction and move with their lists, nothing is encoded again.
          search(..., bitmap=) and search_device(..., d_bitmap=) take a row filter of that call alone, which leaves the handle as it is
  pack_bitmap  a byte or bool mask [n] or [nq, n] -> the LSB-first bits such a call takes, and their stride
  train   (centroids, codebook blob) from ivf.train and pq.train; with residual=True the codebooks are trained on the residuals
"""
import ctypes as C

import numpy as np

from . import _lib, gpu, ivf, pq
from ._ivfbase import IVFBase
from ._rowfilter import RowFilterMixin, pack_bitmap  # noqa: F401  (pack_bitmap: exported here as ivfpq.pack_bitmap)

FLT_MAX = ivf.FLT_MAX


def train(vectors, nlist, M, max_iter=20, seed=0, device=0, residual=False, centroids=None):
    """-> (centroids f32 [nlist, dims], codebook blob): ivf.train for the coarse quantiser, pq.train (K = 256) for the codebooks,
    both over the same rows.  With residual=True the codebooks are pq.train of vectors - centroids[a] (numpy f32 on the host,
    one subtraction a component, as the handle's), a being the k = 1 L2 labels of the rows over a gpu.Index of the centroids in
    order 0 (SEQ).  A handle created with order = 1 may put a row that lies on a boundary between two lists into the other one:
    that row's code is then of a residual the codebooks were not trained on, which bears on quality only, never on exactness.
    centroids [nlist, dims] (say from ivf.train_coarse, which goes past 256 lists) are used as given in place of the coarse
    step, by the residual branch too."""
    v = np.ascontiguousarray(vectors, np.float32)
    if centroids is None:
        centroids = ivf.train(vectors, nlist, max_iter, seed, device=device)
    else:
        centroids = ivf.check_centroids(centroids, nlist, v.shape[-1])
    if residual:
        coarse = gpu.Index(gpu.GPUConfig(DeviceID=device, Dimension=v.shape[1]))
        try:
            coarse.set_order(0)
            coarse.Add(None, centroids)
            a = np.concatenate([coarse.SearchBatch(v[r0:r0 + 65536], 1)[0][:, 0] for r0 in range(0, v.shape[0], 65536)])
        finally:
            coarse.Close()
        v = v - centroids[a]
    blob, _ = pq.train(v, M, 256, max_iter, seed, device=device)
    return centroids, blob


class IVFPQ(ivf.RemovalMixin, RowFilterMixin, IVFBase):
    """lb_gpu_ivfpq: codebooks (the reference's serialised blob, or a pq.PQEncoder whose blob is taken), centroids f32
    [nlist, dims], order 0 SEQ / 1 UNROLL4 of the coarse quantiser (L2).  Under a row filter (RowFilterMixin) the probes stay as
    they are and a search sees the visible rows of the probed lists alone.  residual=True makes a residual handle
    (lb_gpu_ivfpq_new_residual): codes() are then the codes of the rows' residuals, and the codebooks should come from
    train(..., residual=True)."""
    _prefix = "lb_gpu_ivfpq"
    _timing_slots = 5

    def __init__(self, codebooks, centroids, order=0, device=0, lib=None, residual=False):
        self._h = None  # (Close() and __del__ find this when creation fails below)
        buf = bytes(codebooks.blob if isinstance(codebooks, pq.PQEncoder) else codebooks)
        c = np.ascontiguousarray(centroids, np.float32)
        if c.ndim != 2 or c.shape[0] == 0 or c.shape[1] == 0:
            raise ValueError("centroids must be a non-empty [nlist, dims] array")
        if len(buf) >= 12 and int.from_bytes(buf[:4], "little") != c.shape[1]:
            raise ValueError(f"centroids of {c.shape[1]} dimensions, codebooks of {int.from_bytes(buf[:4], 'little')}")
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        new = lib.lb_gpu_ivfpq_new_residual if residual else lib.lb_gpu_ivfpq_new
        h = new(device, buf, len(buf), order, c.shape[0], c.ctypes.data, C.byref(st))
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
        self.residual = bool(lib.lb_gpu_ivfpq_residual(self._h))

    def add(self, vectors, ids=None):
        """assign, encode (on a residual handle: the row less its list's centroid) and append rows [n, dims]; ids (int64 [n]) on
        every add or on none.  Each add rebuilds the lists and the list-major codes of all rows: O(ntotal)."""
        super().add(vectors, ids)

    def codes(self, row0=0, n=None):
        """the codes of rows [row0, row0 + n), insertion order -> uint8 [n, M]"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((max(n, 0), self.m), np.uint8)
        self._check(self._lib.lb_gpu_ivfpq_get_codes(self._h, row0, n, out.ctypes.data))
        return out

    def search(self, queries, k, nprobe, ctx=None, bitmap=None, bitmap_stride=0):
        """-> (labels [nq, k], dist [nq, k]): ascending (ADC distance, row) among the rows of the probed lists, padded -1 / FLT_MAX.
        bitmap: a row filter of this call alone (lb_gpu_ivfpq_search_bitmap_ctx), the LSB-first bits of pack_bitmap over the ntotal
        row positions; bitmap_stride 0: one bitmap for every query, else query q's bits start at byte q * bitmap_stride.  The
        handle, its own filter and nvisible() stay as they are; searches with different bitmaps may run concurrently."""
        return self._search_host("search", self._vectors(queries), k, nprobe, ctx, bitmap, bitmap_stride)

    def search_device(self, nq, d_queries, k, nprobe, d_dist, d_labels, stream=None, ctx=None, d_bitmap=None, nbits=0, bitmap_stride=0):
        """d_bitmap: the call's bitmap in device memory, of nbits == ntotal bits (any byte address)"""
        self._search_dev("search", nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, d_bitmap, nbits, bitmap_stride)

    def search_refine(self, index, queries, k, shortlist, nprobe, order=None, bitmap=None, bitmap_stride=0):
        """The two-stage use the codes exist for, on the device: the ADC k-NN of `shortlist` rows per query among the probed
        lists, then the exact top k of every shortlist on `index` in one call (gpu.Index.Refine; a float32 or float16
        gpu.Index filled in the same row order).  -> (labels [nq, k], dist [nq, k]), padded with -1 / FLT_MAX.  The shortlist
        must hold row positions: a handle that was given ids raises ValueError.  A row filter on this handle shapes the
        shortlist, so the result holds visible rows only; `index` needs no filter.  bitmap, bitmap_stride: a row filter of this
        call alone, as search takes it; it goes to the shortlist search, so the refined result holds rows with a set bit only.
        Removed rows never enter the shortlist
        (it holds live rows only), and `index` treats a position it has removed itself as outside the index.  After compact()
        the positions of this handle are the survivors' new ones: `index` must be compacted over the same removals
        (gpu.Index.Compact is stable too), or the positions no longer correspond."""
        if self._has_ids:
            raise ValueError("search_refine needs row positions: this handle was given ids, which its searches return instead")
        v = self._vectors(queries)
        short, _ = self.search(v, shortlist, nprobe, bitmap=bitmap, bitmap_stride=bitmap_stride)
        return index.Refine(v, short, k, order)

    def last_timing(self):
        """ms of the last profiled search, summed over its batches: (probes, plan, ADC tables, scan, selection).  On a residual
        handle the third is the residual queries and their tables; when one query's tables go in several rounds of slots, the
        rounds after the first are whole in the fourth.  The compaction of the lists under a call's bitmap falls into the
        plan's."""
        return super().last_timing()

    def last_build_timing(self):
        """ms of the last profiled build of the visible lists (a filter call or an add under a filter): its launches alone"""
        out = C.c_float(0)
        self._check(self._lib.lb_gpu_ivfpq_last_build_timing(self._h, C.byref(out)))
        return float(out.value)
