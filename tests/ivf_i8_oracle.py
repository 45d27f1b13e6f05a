"""The semantics of an IVF-Flat handle over int8 rows (include/longbow_gpu.h, lb_gpu_ivf_*: "int8 rows") restated over what the
suite already trusts: the lists and the probes are tests/ivf_oracle.py's over the rows and queries widened to f32 (exact), the
distances are tests/i8_oracle.py's (the reference's DataTypeInt8 kernels), and the result is the canonical top-k, ascending
(distance, row), over the rows of the probed lists, under a mask or not."""
import numpy as np

from tests import i8_oracle as i8
from tests import ivf_oracle as io

F = np.float32


def to_i8(A, scale):
    """a float case of ivf_oracle scaled and rounded into int8"""
    return np.clip(np.rint(np.asarray(A, np.float64) * scale), -128, 127).astype(np.int8)


def assign(oracle, metric, order, X8, C):
    """list of every row: ivf_oracle.assign of the widened rows"""
    return io.assign(oracle, metric, order, X8.astype(F), C)


def search(oracle, metric, order, Q8, X8, C, lists, k, nprobe, ids=None, mask=None):
    """-> (labels [nq, k], dist [nq, k], rows scanned per query [nq]); mask: a row filter, a hidden row being a row in no list"""
    lists = np.asarray(lists) if mask is None else np.where(np.asarray(mask) != 0, lists, -1)
    W = Q8.astype(F)
    labels = np.empty((Q8.shape[0], k), np.int64)
    dist = np.empty((Q8.shape[0], k), F)
    scanned = np.empty(Q8.shape[0], np.int64)
    every = i8.distances(metric, Q8, X8)  # (of every pair, once: the cases are small)
    for j in range(Q8.shape[0]):
        rows = io.probed_rows(lists, io.probes(oracle, metric, order, W[j], C, nprobe))
        scanned[j] = rows.size
        lab, dist[j] = i8.topk(every[j, rows], k, rows)
        labels[j] = lab if ids is None else np.where(lab >= 0, np.asarray(ids)[np.clip(lab, 0, None)], -1)
    return labels, dist, scanned
