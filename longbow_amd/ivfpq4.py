"""IVF-PQ4 on the GPU (lb_gpu_ivfpq4_*): the coarse partition of ivf.IVFFlat over the packed 4-bit codes of pq4.PQ4Encoder.

What ivfpq.IVFPQ is at K = 256 this is at K = 16: a row costs ceil(M / 2) bytes, a query's ADC table M * 64 bytes instead of
M * 1024.  Given the codes and the probed lists nothing is approximate: the result is the exact ADC k-NN among the live, visible
rows of the probed lists, bit for bit in pq4.PQ4Encoder's arithmetic (Encode's encodeSequential branch, BuildADCTable and
ADCDistance at stride 16), and with every list probed a plain handle equals pq4.PQ4Encoder.Search over the same codes.  Plain
and residual handles are ivfpq's two kinds; on a residual handle the table per probed list is sixteen times cheaper to build and
hold than there.  include/longbow_gpu.h states the semantics.

  IVFPQ4  the handle, with every method of ivfpq.IVFPQ: add / search / search_device (bitmap=, d_bitmap=) / search_refine /
          codes / assignments / list_sizes / centroids / last_search_stats, the row filter, removal and compact()
  train   (centroids, codebook blob) from ivf.train and pq.train at K = 16; with residual=True the codebooks are trained on the residuals
"""
import ctypes as C

import numpy as np

from . import _lib, gpu, ivf, ivfpq, pq
from ._rowfilter import pack_bitmap  # noqa: F401  (exported here as ivfpq4.pack_bitmap)

K = 16
FLT_MAX = ivfpq.FLT_MAX


def train(vectors, nlist, M, max_iter=20, seed=0, device=0, residual=False, centroids=None):
    """-> (centroids f32 [nlist, dims], codebook blob): what ivfpq.train does, with pq.train at K = 16 for the codebooks.  The
    coarse centroids are ivf.train's (or `centroids` as given); with residual=True the codebooks are pq.train of
    vectors - centroids[a], a being the k = 1 L2 labels of the rows over a gpu.Index of the centroids in order 0 (SEQ)."""
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
    blob, _ = pq.train(v, M, K, max_iter, seed, device=device)
    return centroids, blob


class IVFPQ4(ivfpq.IVFPQ):
    """lb_gpu_ivfpq4: codebooks with K = 16 (the reference's serialised blob, or a pq4.PQ4Encoder / pq.PQEncoder whose blob is
    taken), centroids f32 [nlist, dims], order 0 SEQ / 1 UNROLL4 of the coarse quantiser (L2).  residual=True makes a residual
    handle (lb_gpu_ivfpq4_new_residual), whose codebooks should come from train(..., residual=True).  codes() are M bytes a
    row, each below 16, as pq4.PQ4Encoder.get_codes returns them; in HBM two share a byte."""
    _prefix = "lb_gpu_ivfpq4"

    def __init__(self, codebooks, centroids, order=0, device=0, lib=None, residual=False):
        self._h = None  # (Close() and __del__ find this when creation fails below)
        buf = bytes(codebooks.blob if hasattr(codebooks, "blob") else codebooks)
        c = np.ascontiguousarray(centroids, np.float32)
        if c.ndim != 2 or c.shape[0] == 0 or c.shape[1] == 0:
            raise ValueError("centroids must be a non-empty [nlist, dims] array")
        if len(buf) >= 12 and int.from_bytes(buf[:4], "little") != c.shape[1]:
            raise ValueError(f"centroids of {c.shape[1]} dimensions, codebooks of {int.from_bytes(buf[:4], 'little')}")
        lib = lib or _lib.require_gpu(device)
        st = C.c_int(0)
        new = lib.lb_gpu_ivfpq4_new_residual if residual else lib.lb_gpu_ivfpq4_new
        h = new(device, buf, len(buf), order, c.shape[0], c.ctypes.data, C.byref(st))
        if not h:
            if st.value == 1:
                raise ValueError("invalid PQ data")  # persistence.go:39-56 error cases, as pq.PQEncoder
            _lib.check(st.value or 7)
        self._lib = lib
        self._h = C.c_void_p(h)
        self.device = device
        self.nlist, self.dims = c.shape
        self.m = lib.lb_gpu_ivfpq4_m(self._h)
        self.order = order
        self.residual = bool(lib.lb_gpu_ivfpq4_residual(self._h))

    def codes(self, row0=0, n=None):
        """the codes of rows [row0, row0 + n), insertion order -> uint8 [n, M], one code a byte"""
        n = self.ntotal - row0 if n is None else n
        out = np.empty((max(n, 0), self.m), np.uint8)
        self._check(self._lib.lb_gpu_ivfpq4_get_codes(self._h, row0, n, out.ctypes.data))
        return out

    def last_build_timing(self):
        """ms of the last profiled build of the visible lists (a filter call or an add under a filter): its launches alone"""
        out = C.c_float(0)
        self._check(self._lib.lb_gpu_ivfpq4_last_build_timing(self._h, C.byref(out)))
        return float(out.value)
