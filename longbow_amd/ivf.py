"""IVF-Flat on the GPU (lb_gpu_ivf_*): the index type the reference names -- IndexTypeIVFFlat = "ivf_flat", IVFFlatConfig{NClusters,
NProbe} (internal/store/pluggable_index.go:18-25,100-104) -- and leaves a stub (pluggable_index_adapters.go:116-223).

A coarse partition of the rows lets a query skip most of them.  Nothing is approximate except which lists are probed: given the
probed lists the result is the exact k-NN among their rows, bit for bit in the reference's distance arithmetic, and with every
list probed it equals gpu.Index.Search.  include/longbow_gpu.h states the semantics.

  IVFFlat        the handle: centroids given at creation, add / search / list_sizes / assignments / last_search_stats, and the
                 row filter (set_filter / filter_column / nvisible), removal (remove / remove_rows / remove_device / nlive /
                 ndeleted) and compact(); dtype=DataType.Float16 holds the rows as float16, 2 bytes an
                 element, and answers as a float32 handle over the widened rows does, bit for bit.  search(..., bitmap=) and
                 search_device(..., d_bitmap=) take a row filter of that call alone, which leaves the handle as it is
  pack_bitmap    a byte or bool mask [n] or [nq, n] -> the LSB-first bits such a call takes, and their stride
  IVFFlatInt8    the same handle over signed int8 rows (lb_gpu_ivf_new_i8), one byte an element, searched with int8 queries in
                 the reference's DataTypeInt8 arithmetic (L2 and dot); with every list probed it equals the flat int8 index
  IVFFlatIndex   the reference's PluggableVectorIndex surface over it: rows are buffered until Build()
  train          TrainKMeans on the GPU (pq.train with M = 1): nlist <= 256 centroids of f32 rows
  train_coarse   the same TrainKMeans for any nlist up to 65,536 (lb_gpu_ivf_train): a tiled exact f32 E-step over whole rows,
                 the lists' own counting sort for the ordering; equal to train bit for bit where both apply
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, pq
from ._ivfbase import IVFBase
from ._rowfilter import RowFilterMixin, pack_bitmap  # noqa: F401  (pack_bitmap: exported here as ivf.pack_bitmap)
from .gpu import DataType

FLT_MAX = np.float32(3.4028234663852886e38)
MAX_NLIST = 65536
TRAIN_MAX_NLIST = 256  # lb_gpu_pq_train's K


def train(vectors, nlist, max_iter=20, seed=0, init_rows=None, device=0):
    """TrainKMeans(vectors, n, dims, nlist, max_iter) (internal/pq/kmeans.go:64-151) on the GPU -> centroids f32 [nlist, dims].
    It is pq.train with M = 1 and K = nlist, the blob's 12-byte header stripped, and inherits that call's K <= 256; centroids
    from elsewhere may have any nlist up to 65,536.  max_iter = 0 returns the init rows."""
    if nlist > TRAIN_MAX_NLIST:
        raise ValueError(f"ivf.train takes nlist <= {TRAIN_MAX_NLIST} (lb_gpu_pq_train's K), got {nlist}")
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2 or v.shape[0] == 0:
        raise ValueError("empty training data")
    rows = None if init_rows is None else np.ascontiguousarray(init_rows, np.int64).reshape(1, nlist)
    blob, _ = pq.train(v, 1, nlist, max_iter, seed, rows, device)
    return np.frombuffer(blob[12:], "<f4").reshape(nlist, v.shape[1]).copy()


def train_device(n, d_vectors, dims, nlist, max_iter=20, seed=0, init_rows=None, device=0):
    """train() over n rows already resident on the device (d_vectors: device address); init_rows stays a host array"""
    if nlist > TRAIN_MAX_NLIST:
        raise ValueError(f"ivf.train takes nlist <= {TRAIN_MAX_NLIST} (lb_gpu_pq_train's K), got {nlist}")
    rows = None if init_rows is None else np.ascontiguousarray(init_rows, np.int64).reshape(1, nlist)
    blob, _ = pq.train_device(n, d_vectors, dims, 1, nlist, max_iter, seed, rows, device)
    return np.frombuffer(blob[12:], "<f4").reshape(nlist, dims).copy()


def _coarse_args(n, dims, nlist, init_rows):
    """what needs no device: the ValueErrors of train_coarse* and the call's host buffers"""
    if not 1 <= nlist <= MAX_NLIST:
        raise ValueError(f"ivf.train_coarse takes nlist in 1..{MAX_NLIST}, got {nlist}")
    if n <= 0 or dims <= 0:
        raise ValueError("empty training data")
    rows = None
    if init_rows is not None:
        rows = np.ascontiguousarray(init_rows, np.int64)
        if rows.shape != (nlist,):
            raise ValueError(f"init_rows of shape {rows.shape}, want ({nlist},)")
    return np.empty((nlist, dims), np.float32), np.zeros(1, np.int32), rows


def train_coarse(vectors, nlist, max_iter=20, seed=0, init_rows=None, device=0, ctx=None, return_iters=False):
    """TrainKMeans(vectors, n, dims, nlist, max_iter) on the GPU for any nlist in 1..65,536 (lb_gpu_ivf_train) -> centroids f32
    [nlist, dims], with return_iters the pair (centroids, iterations run).  The contract is train()'s; for nlist <= 256 the
    bytes and the iteration count equal train()'s.  init_rows [nlist]: rows whose copies are the first centroids (None: drawn
    from seed).  max_iter = 0 returns the init rows."""
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2 or v.shape[0] == 0:
        raise ValueError("empty training data")
    n, dims = v.shape
    cent, iters, rows = _coarse_args(n, dims, nlist, init_rows)
    lib = _lib.require_gpu(device)
    _lib.check(lib.lb_gpu_ivf_train(device, dims, nlist, n, v.ctypes.data, max_iter, seed, rows.ctypes.data if rows is not None else None,
                                    cent.ctypes.data, iters.ctypes.data, ctx._h if ctx is not None else None))
    return (cent, int(iters[0])) if return_iters else cent


def train_coarse_device(n, d_vectors, dims, nlist, max_iter=20, seed=0, init_rows=None, device=0, ctx=None, return_iters=False,
                        stream=None):
    """train_coarse() over n rows already resident on the device (d_vectors: device address); init_rows stays a host array and
    the centroids come back to the host"""
    cent, iters, rows = _coarse_args(n, dims, nlist, init_rows)
    lib = _lib.require_gpu(device)
    _lib.check(lib.lb_gpu_ivf_train_device(device, dims, nlist, n, d_vectors, max_iter, seed, rows.ctypes.data if rows is not None else None,
                                           cent.ctypes.data, iters.ctypes.data, stream, ctx._h if ctx is not None else None))
    return (cent, int(iters[0])) if return_iters else cent


def check_centroids(centroids, nlist, dims):
    """centroids given to a train(..., centroids=) in place of the coarse step -> f32 [nlist, dims], the array itself when it is one"""
    c = np.ascontiguousarray(centroids, np.float32)
    if c.shape != (nlist, dims):
        raise ValueError(f"centroids of shape {c.shape}, want {(nlist, dims)}")
    return c


def rows_f16(vectors, dims):
    """rows for a float16 handle -> np.float16 [n, dims], contiguous; np.float16 arrays only"""
    v = np.asarray(vectors)
    if v.dtype != np.float16:
        raise TypeError(f"a float16 index takes np.float16 arrays, got {v.dtype}")
    v = np.ascontiguousarray(v)
    v = v.reshape(-1, v.shape[-1]) if v.size else v.reshape(0, dims)
    if v.shape[1] != dims:
        raise ValueError(f"vector dimension {v.shape[1]} does not match {dims}")
    return v


class RemovalMixin:
    """<prefix>_remove* / _nlive / _ndeleted / _compact on a handle of IVFBase, resolved by the handle's prefix: written once for
    IVFFlat, IVFFlatInt8 and the code handles ivfpq.IVFPQ and ivfsq8.IVFSQ8 (whose "rows" are their codes)"""

    def _remove(self, entry, values):
        values = np.ascontiguousarray(values, np.int64).reshape(-1)
        removed = C.c_int64(0)
        self._check(self._fn(entry)(self._h, values.size, values.ctypes.data if values.size else None, C.byref(removed)))
        return int(removed.value)

    def remove(self, labels):
        """Remove the rows with these labels (the values search returns: the ids given to add, else row positions) -> the number
        of rows newly removed.  Every live row under a given id goes; unknown labels, -1, repeats and rows already removed are
        ignored.  Searches stop returning them at once; the rows keep their positions, their lists and their memory until
        compact()."""
        return self._remove("remove", labels)

    def remove_rows(self, rows):
        """Remove by row position, whether or not the handle holds ids"""
        return self._remove("remove_rows", rows)

    def remove_device(self, n, d_labels):
        """remove() of n int64 labels in device memory"""
        removed = C.c_int64(0)
        self._check(self._fn("remove_device")(self._h, n, d_labels, C.byref(removed)))
        return int(removed.value)

    def compact(self):
        """Drop the removed rows physically, keeping the survivors' order and their lists -> old_rows int64 [nlive]: each
        survivor's former position.  ids are kept; a handle without ids labels by the new positions from here on.  A filter in
        force survives."""
        old = np.empty(self.nlive(), np.int64)
        self._check(self._fn("compact")(self._h, old.ctypes.data, old.size))
        return old

    def nlive(self):
        """rows a search can return without a filter: ntotal - ndeleted()"""
        return int(self._fn("nlive")(self._h))

    def ndeleted(self):
        """removed rows the handle still holds; ntotal, list_sizes and assignments count them until compact()"""
        return int(self._fn("ndeleted")(self._h))


class IVFFlat(RemovalMixin, RowFilterMixin, IVFBase):
    """lb_gpu_ivf: metric 0 L2 / 1 cosine / 2 dot, order 0 SEQ / 1 UNROLL4, centroids f32 [nlist, dims].  Under a row filter
    (RowFilterMixin) the probes stay as they are and a search sees the visible rows of the probed lists alone.
    dtype: DataType.Float32, or DataType.Float16 (lb_gpu_ivf_new_f16): the rows are held as float16.  Such a handle's add takes
    np.float16 arrays only, as gpu.Index does for its Float16 type (converting other data here would change the vectors
    silently), and add_device fp16 rows; the centroids and the queries stay float32 (float16 queries are widened here, which
    is exact)."""
    _prefix = "lb_gpu_ivf"
    _timing_slots = 4

    def __init__(self, centroids, metric=0, order=0, device=0, lib=None, dtype=DataType.Float32):
        self._h = None  # (Close() and __del__ find this when creation fails below)
        c = np.ascontiguousarray(centroids, np.float32)
        if c.ndim != 2 or c.shape[0] == 0 or c.shape[1] == 0:
            raise ValueError("centroids must be a non-empty [nlist, dims] array")
        if dtype not in (DataType.Float32, DataType.Float16):
            raise ValueError(f"an IVF-Flat handle holds float32 (0) or float16 (1) rows, got data type {dtype}"
                             + (": int8 rows are IVFFlatInt8's" if dtype == DataType.Int8 else ""))
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        new = lib.lb_gpu_ivf_new_f16 if dtype == DataType.Float16 else lib.lb_gpu_ivf_new
        h = new(device, c.shape[1], metric, order, c.shape[0], c.ctypes.data, C.byref(st))
        if not h:
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.device = device
        self.nlist, self.dims = c.shape
        self.metric, self.order = metric, order
        self._f16 = dtype == DataType.Float16

    @property
    def dtype(self):
        """0 float32, 1 float16 (lb_gpu_ivf_dtype)"""
        return int(self._lib.lb_gpu_ivf_dtype(self._h))

    def add(self, vectors, ids=None):
        if not self._f16:
            return super().add(vectors, ids)
        self._add(rows_f16(vectors, self.dims), ids, "add_f16")

    def add_device(self, n, d_vectors, d_ids=None):
        """d_vectors: f32 rows, fp16 rows on a float16 handle"""
        self._check(self._fn("add_f16_device" if self._f16 else "add_device")(self._h, n, d_vectors, d_ids))
        self._has_ids = self._has_ids or d_ids is not None

    def search(self, queries, k, nprobe, ctx=None, bitmap=None, bitmap_stride=0):
        """As IVFBase.search.  bitmap: a row filter of this call alone (lb_gpu_ivf_search_bitmap_ctx), the LSB-first bits of
        pack_bitmap over the ntotal row positions; bitmap_stride 0: one bitmap for every query, else query q's bits start at byte
        q * bitmap_stride.  The handle, its own filter and nvisible() stay as they are; searches with different bitmaps may run
        at the same time."""
        return self._search_host("search", self._vectors(queries), k, nprobe, ctx, bitmap, bitmap_stride)

    def search_device(self, nq, d_queries, k, nprobe, d_dist, d_labels, stream=None, ctx=None, d_bitmap=None, nbits=0, bitmap_stride=0):
        """d_bitmap: the call's bitmap in device memory, of nbits == ntotal bits (any byte address)"""
        self._search_dev("search", nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, d_bitmap, nbits, bitmap_stride)

    def last_timing(self):
        """ms of the last profiled search, summed over its batches: (probes, plan, list scan, selection); the compaction under a
        call's bitmap falls into the plan's"""
        return super().last_timing()

    def last_build_timing(self):
        """ms of the last profiled build of the visible lists (a filter call or an add under a filter): its launches alone"""
        out = C.c_float(0)
        self._check(self._lib.lb_gpu_ivf_last_build_timing(self._h, C.byref(out)))
        return float(out.value)


def rows_i8(vectors, dims):
    """rows or queries for an int8 handle -> np.int8 [n, dims], contiguous; np.int8 arrays only"""
    v = np.asarray(vectors)
    if v.dtype != np.int8:
        raise TypeError(f"an int8 index takes np.int8 arrays, got {v.dtype}")
    v = np.ascontiguousarray(v)
    v = v.reshape(-1, v.shape[-1]) if v.size else v.reshape(0, dims)
    if v.shape[1] != dims:
        raise ValueError(f"vector dimension {v.shape[1]} does not match {dims}")
    return v


class IVFFlatInt8(RemovalMixin, RowFilterMixin, IVFBase):
    """lb_gpu_ivf over signed int8 rows (lb_gpu_ivf_new_i8): metric 0 L2 / 2 dot, centroids f32 [nlist, dims]; order 0 SEQ /
    1 UNROLL4 is the coarse index's and decides lists and probes alone.  add, search and their device-pointer forms take int8
    rows and int8 queries, np.int8 arrays only (converting other data here would change the vectors silently).  The distances are
    the flat int8 index's (gpu.Index with DataType.Int8), and with every list probed so is the result.  Row filters as on
    IVFFlat."""
    _prefix = "lb_gpu_ivf"
    _timing_slots = 4

    def __init__(self, centroids, metric=0, order=0, device=0, lib=None):
        self._h = None  # (Close() and __del__ find this when creation fails below)
        c = np.ascontiguousarray(centroids, np.float32)
        if c.ndim != 2 or c.shape[0] == 0 or c.shape[1] == 0:
            raise ValueError("centroids must be a non-empty [nlist, dims] array")
        if metric == 1:
            raise ValueError("an int8 IVF-Flat handle takes metric 0 (L2) or 2 (dot): the reference has no int8 cosine kernel")
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        h = lib.lb_gpu_ivf_new_i8(device, c.shape[1], metric, order, c.shape[0], c.ctypes.data, C.byref(st))
        if not h:
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.device = device
        self.nlist, self.dims = c.shape
        self.metric, self.order = metric, order

    @property
    def dtype(self):
        """2 (lb_gpu_ivf_dtype)"""
        return int(self._lib.lb_gpu_ivf_dtype(self._h))

    def add(self, vectors, ids=None):
        self._add(rows_i8(vectors, self.dims), ids, "add_i8")

    def add_device(self, n, d_vectors, d_ids=None):
        """d_vectors: int8 rows"""
        self._check(self._fn("add_i8_device")(self._h, n, d_vectors, d_ids))
        self._has_ids = self._has_ids or d_ids is not None

    def search(self, queries, k, nprobe, ctx=None, bitmap=None, bitmap_stride=0):
        """int8 queries -> (labels [nq, k], dist [nq, k]), as IVFFlat.search (bitmap: lb_gpu_ivf_search_i8_bitmap_ctx)"""
        return self._search_host("search_i8", rows_i8(queries, self.dims), k, nprobe, ctx, bitmap, bitmap_stride)

    def search_device(self, nq, d_queries, k, nprobe, d_dist, d_labels, stream=None, ctx=None, d_bitmap=None, nbits=0, bitmap_stride=0):
        """d_queries: int8 [nq, dims]; d_bitmap as IVFFlat.search_device"""
        self._search_dev("search_i8", nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, d_bitmap, nbits, bitmap_stride)

    def last_timing(self):
        """ms of the last profiled search, summed over its batches: (probes, plan, list scan, selection)"""
        return super().last_timing()

    def last_build_timing(self):
        """ms of the last profiled build of the visible lists (a filter call or an add under a filter): its launches alone"""
        out = C.c_float(0)
        self._check(self._lib.lb_gpu_ivf_last_build_timing(self._h, C.byref(out)))
        return float(out.value)


@dataclass
class IVFFlatConfig:
    """pluggable_index.go:100-104"""
    NClusters: int = 256
    NProbe: int = 8


class IVFFlatIndex:
    """The reference's IVFFlatIndex surface (pluggable_index_adapters.go:116-223) with an index behind it.  Before Build() rows are
    buffered on the host, as the stub keeps them in its map; Build() takes the centroids as given, or trains them on the buffered
    rows (ivf.train up to 256 lists, ivf.train_coarse beyond), creates the handle and adds the rows; after it, adds go straight
    to the handle.  data_type=DataType.Float16: the rows are np.float16 arrays, buffered and stored as such; Build() trains on the
    widened rows."""

    def __init__(self, dimension, config=None, metric=0, order=0, device=0, centroids=None, train_iters=20, seed=0,
                 data_type=DataType.Float32):
        if dimension <= 0:
            raise ValueError(f"dimension must be positive, got {dimension}")
        if data_type not in (DataType.Float32, DataType.Float16):
            raise ValueError(f"an IVF-Flat handle holds float32 (0) or float16 (1) rows, got data type {data_type}"
                             + (": int8 rows are IVFFlatInt8's, outside this float-only surface" if data_type == DataType.Int8 else ""))
        self.data_type = data_type
        self._np = np.float16 if data_type == DataType.Float16 else np.float32
        self.config = config or IVFFlatConfig()
        if self.config.NClusters <= 0 or self.config.NProbe <= 0:
            raise ValueError("NClusters and NProbe must be positive")
        _lib.require_gpu(device)
        self.dimension, self.metric, self.order, self.device = dimension, metric, order, device
        self._centroids = None if centroids is None else np.ascontiguousarray(centroids, np.float32)
        if self._centroids is not None and self._centroids.shape != (self.config.NClusters, dimension):
            raise ValueError(f"centroids of shape {self._centroids.shape}, config asks for {(self.config.NClusters, dimension)}")
        self._train_iters, self._seed = train_iters, seed
        self._ids, self._rows = [], []
        self._h = None

    def Type(self):
        return "ivf_flat"

    def Dimension(self):
        return self.dimension

    def Size(self):
        return self._h.ntotal if self._h is not None else sum(r.shape[0] for r in self._rows)

    Len = Size

    def NeedsBuild(self):
        return True  # IVF requires training / clustering (pluggable_index_adapters.go:143-145)

    def AddBatch(self, ids, vectors):
        if self._np is np.float16:
            v = rows_f16(vectors, self.dimension)
        else:
            v = np.ascontiguousarray(vectors, np.float32).reshape(-1, self.dimension)
        i = np.ascontiguousarray(ids, np.int64).reshape(-1)
        if i.size != v.shape[0]:
            raise ValueError(f"{i.size} ids for {v.shape[0]} rows")
        if self._h is not None:
            self._h.add(v, i)
        else:
            self._ids.append(i.copy())
            self._rows.append(v.copy())

    def Add(self, id, vector):
        self.AddBatch([id], np.asarray(vector, None if self._np is np.float16 else np.float32).reshape(1, -1))

    def Build(self):
        if self._h is not None:
            return
        rows = np.concatenate(self._rows) if self._rows else np.empty((0, self.dimension), self._np)
        ids = np.concatenate(self._ids) if self._ids else np.empty(0, np.int64)
        if self._centroids is None:
            fit = train if self.config.NClusters <= TRAIN_MAX_NLIST else train_coarse
            self._centroids = fit(np.ascontiguousarray(rows, np.float32), self.config.NClusters, self._train_iters, self._seed, device=self.device)
        self._h = IVFFlat(self._centroids, self.metric, self.order, self.device, dtype=self.data_type)
        if rows.shape[0]:
            self._h.add(rows, ids)
        self._ids, self._rows = [], []

    def _built(self):
        if self._h is None:
            raise RuntimeError("ivf_flat: Build() before Search()")
        return self._h

    def SearchBatch(self, queries, k, nprobe=None, bitmap=None, bitmap_stride=0):
        """-> (ids [nq, k], distances [nq, k]), padded -1 / FLT_MAX.  bitmap: the reference's SearchVectorsWithBitmap, a filter of
        this call alone over the row positions (pack_bitmap), one for every query or with bitmap_stride one a query"""
        return self._built().search(queries, k, self.config.NProbe if nprobe is None else nprobe, bitmap=bitmap, bitmap_stride=bitmap_stride)

    def Search(self, query, k, nprobe=None, bitmap=None):
        ids, dist = self.SearchBatch(np.asarray(query, np.float32).reshape(1, -1), k, nprobe, bitmap=bitmap)
        return ids[0], dist[0]

    def search_device(self, nq, d_queries, k, d_dist, d_labels, nprobe=None, stream=None, ctx=None):
        self._built().search_device(nq, d_queries, k, self.config.NProbe if nprobe is None else nprobe, d_dist, d_labels, stream, ctx)

    def list_sizes(self):
        return self._built().list_sizes()

    def assignments(self, row0=0, n=None):
        return self._built().assignments(row0, n)

    def last_search_stats(self):
        return self._built().last_search_stats()

    def set_filter(self, mask):
        self._built().set_filter(mask)

    def filter_column(self, column, value, op, valid=None, combine=False, validity_offset=0):
        self._built().filter_column(column, value, op, valid=valid, combine=combine, validity_offset=validity_offset)

    def nvisible(self):
        return self._built().nvisible()

    def Remove(self, ids):
        """the reference's Delete / DeleteBatch: the rows under these ids go -> the number newly removed.  Size() keeps counting
        them until Compact()."""
        return self._built().remove(ids)

    def Compact(self):
        """-> each survivor's former position"""
        return self._built().compact()

    def nlive(self):
        return self._built().nlive()

    def ndeleted(self):
        return self._built().ndeleted()

    def Save(self, path):
        raise NotImplementedError("ivf_flat: Save is not implemented (the reference's writes a marker file only)")

    def Load(self, path):
        raise NotImplementedError("ivf_flat: Load is not implemented (the reference's reads a marker file only)")

    def Close(self):
        if self._h is not None:
            self._h.Close()
            self._h = None
