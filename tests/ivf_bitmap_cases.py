"""The row bitmap given with a search call on the IVF-Flat handle (include/longbow_gpu.h, lb_gpu_ivf_*: "call bitmap") restated for
the tests: how a mask becomes the bits and back, and the shapes tests/test_ivf_bitmap_semantics.py (CPU: the statement is pinned
on them) and tests/test_gpu_ivf_bitmap.py (GPU) share.

The expected result needs no oracle of its own: a search under a bitmap is tests/ivf_filter_cases.search_filtered with the unpacked
bits as the mask, ANDed with the handle's own mask and with liveness where a test sets those; with a stride it is one such search
per query."""
import numpy as np

from tests import ivf_filter_cases as fc

STEP = 2048                                            # IVF_CALL_STEP_ROWS: list positions a compaction workgroup takes per step
STEP_COUNTS = (3, STEP - 1, STEP, STEP + 1, 2 * STEP + 1, 3 * STEP)   # rows per list of the step-edge case
STEP_KEEP = (0, 1, STEP - 1, STEP, STEP + 1, 2 * STEP + 1)            # rows per list that the bitmap leaves


def nbytes(n):
    return (n + 7) // 8


def pack(mask):
    """0/1 (or any byte) mask [n] -> uint8 [ceil(n / 8)]: row r is bit r & 7 of byte r >> 3, a non-zero byte being a set bit; the
    bits past n - 1 in the last byte are zero.  Written out bit by bit: what longbow_amd.ivf.pack_bitmap must give."""
    mask = np.asarray(mask).reshape(-1)
    out = np.zeros(nbytes(mask.size), np.uint8)
    for r in np.flatnonzero(mask != 0):
        out[r >> 3] |= np.uint8(1 << (r & 7))
    return out


def unpack(bits, n):
    """the first n bits of uint8 `bits` -> 0/1 mask [n]; bytes and bits past them are not looked at"""
    bits = np.asarray(bits, np.uint8).reshape(-1)
    r = np.arange(n)
    return ((bits[r >> 3] >> (r & 7).astype(np.uint8)) & 1).astype(np.uint8)


def pack_rows(masks, stride=None, fill=0):
    """masks [nq, n] -> uint8 [nq, stride] (stride >= ceil(n / 8), default exactly that), the bytes behind each bitmap being `fill`"""
    masks = np.asarray(masks)
    nq, n = masks.shape
    stride = nbytes(n) if stride is None else stride
    assert stride >= nbytes(n)
    out = np.full((nq, stride), fill, np.uint8)
    for q in range(nq):
        out[q, :nbytes(n)] = pack(masks[q])
    return out


def per_query_masks(nq, n, seed=12):
    """nq different masks over n rows: the first all zero, the second all one, then densities from 1 % to 90 %, each with row
    q % n set and the row behind it clear, so that none is empty or full"""
    rng = np.random.default_rng(seed)
    m = np.zeros((nq, n), np.uint8)
    m[1] = 1
    for q in range(2, nq):
        m[q] = rng.random(n) < (0.01, 0.1, 0.5, 0.9)[q % 4]
        m[q, q % n], m[q, (q + 1) % n] = 1, 0
    return m


def search_bitmap(oracle, metric, order, Q, X, C, lists, bits, k, nprobe, ids=None, also=None):
    """search_filtered under the unpacked bits (ANDed with the 0/1 mask `also`: the handle's filter, liveness)
    -> (labels, dist, visible rows scanned per query)"""
    m = unpack(bits, X.shape[0])
    if also is not None:
        m = m & (np.asarray(also) != 0)
    return fc.search_filtered(oracle, metric, order, Q, X, C, lists, m, k, nprobe, ids=ids)


def search_strided(oracle, metric, order, Q, X, C, lists, bits2d, k, nprobe, ids=None):
    """query q under bits2d[q]: one single-bitmap search per query"""
    labels = np.empty((Q.shape[0], k), np.int64)
    dist = np.empty((Q.shape[0], k), np.float32)
    scanned = np.empty(Q.shape[0], np.int64)
    for q in range(Q.shape[0]):
        l, d, s = search_bitmap(oracle, metric, order, Q[q:q + 1], X, C, lists, bits2d[q], k, nprobe, ids=ids)
        labels[q], dist[q], scanned[q] = l[0], d[0], s[0]
    return labels, dist, scanned
