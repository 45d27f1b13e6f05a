"""The row filter of the code indexes and of the IVF indexes, shared by bq.py, sq8.py, pq.py, ivf.py and ivfpq.py, and the packing
of a row bitmap given with a search call (gpu.pack_bitmap, ivf.pack_bitmap)."""
import numpy as np


def pack_bitmap(mask):
    """A byte or bool mask over the row positions, [n] or [nq, n] (a row is visible iff its value is non-zero) -> (bits, stride):
    the bits least significant first as in an Arrow validity buffer, row r at bits[r >> 3] >> (r & 7) & 1, as uint8 [ceil(n / 8)]
    with stride 0, or [nq, ceil(n / 8)] with the bytes of one row as the stride.  What ivf.IVFFlat.search(bitmap=, bitmap_stride=)
    takes; gpu.Index.Search / SearchBatch(bitmap=) take the bits of the [n] form (one bitmap per call, no stride)."""
    m = np.asarray(mask) != 0
    if m.ndim not in (1, 2):
        raise ValueError(f"a mask is [n] or [nq, n], got {m.ndim} dimensions")
    bits = np.ascontiguousarray(np.packbits(m, axis=-1, bitorder="little"))
    return bits, (0 if m.ndim == 1 else bits.shape[1])


class RowFilterMixin:
    """The row filter of a code index (bq.BQEncoder, sq8.SQ8Encoder, pq.PQEncoder): what gpu.Index offers on the f32 index, on the
    <_prefix>_set_filter / _filter_int64 / _filter_float32 / _nvisible entry points.  With a filter every search returns the
    exact k-NN among the visible rows (labels stay corpus rows); rows added later are visible; the calls that address rows
    directly ignore it."""
    _prefix = None  # "lb_gpu_bq" / "lb_gpu_sq8" / "lb_gpu_pq" / "lb_gpu_ivf" / "lb_gpu_ivfpq" (ivf.IVFFlat, ivfpq.IVFPQ: the visible rows
    #                 of the probed lists)

    def set_filter(self, mask):
        """mask: ntotal bytes, a row is visible iff its byte is non-zero; None clears the filter"""
        fn = getattr(self._lib, self._prefix + "_set_filter")
        if mask is None:
            self._check(fn(self._h, None, 0))
            return
        mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        self._check(fn(self._h, mask.ctypes.data, mask.size))

    def filter_column(self, column, value, op, valid=None, combine=False, validity_offset=0):
        """Evaluate `column OP value` on the device into the row mask.  column: int64 or float32, ntotal values; op: a
        simd.CompareOp value or a query.Filter operator string; valid: an Arrow validity bitmap (LSB first, row i is bit
        i + validity_offset; nulls never match) or None; combine=True ANDs into the current mask (replaces it when there is none)."""
        from .simd import parse_operator
        op = int(parse_operator(op))
        column = np.ascontiguousarray(column).reshape(-1)
        vptr = None
        if valid is not None:
            valid = np.ascontiguousarray(valid if isinstance(valid, np.ndarray) else np.frombuffer(valid, np.uint8), np.uint8)
            vptr = valid.ctypes.data
        if column.dtype == np.int64:
            rc = getattr(self._lib, self._prefix + "_filter_int64")(self._h, column.ctypes.data, column.size, int(value), op, vptr,
                                                                    validity_offset, 1 if combine else 0)
        elif column.dtype == np.float32:
            rc = getattr(self._lib, self._prefix + "_filter_float32")(self._h, column.ctypes.data, column.size, float(value), op, vptr,
                                                                      validity_offset, 1 if combine else 0)
        else:
            raise TypeError(f"unsupported filter column type {column.dtype} (int64 / float32)")
        self._check(rc)

    def nvisible(self):
        """rows a search sees: ntotal without a filter"""
        return int(getattr(self._lib, self._prefix + "_nvisible")(self._h))
