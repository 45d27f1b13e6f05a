"""The row bitmap given with a search call on the flat index (include/longbow_gpu.h, lb_gpu_index_*: "call bitmap") restated for
the tests: the expected result and the shapes tests/test_index_bitmap_semantics.py (CPU: the statement is pinned on them) and
tests/test_gpu_index_bitmap.py (GPU) share.

The expected result needs no oracle of its own: a search under a bitmap is oracle.search_batch with the unpacked bits as the mask,
ANDed with the handle's own mask and with liveness where a test sets those.  Packing and unpacking are tests/ivf_bitmap_cases.py's,
written out bit by bit there."""
import numpy as np

from tests import ivf_bitmap_cases as bc
from tests import row_view_cases as rc

BLOCK = rc.CP_ROWS                            # positions per workgroup of the pass that turns bits into the call's view
EDGE_N = (1, 7, 8, 9, 2047, 2048, 2049)       # one byte and less, the byte's edge, the block's edge
ROUND_TRIP_N = (1, 7, 8, 9, 2049)
MAX_PCT = 95                                  # LB_ROWMAP_MAX_PCT: the view rule's edge


def effective_mask(bits, n, also=None):
    """0/1 mask [n] of the rows a call under `bits` sees: bit r set, and (also: the handle's filter bytes, liveness) non-zero"""
    m = bc.unpack(bits, n)
    if also is not None:
        m = m & (np.asarray(also).reshape(-1)[:n] != 0).astype(np.uint8)
    return m


def search_bitmap(oracle, metric, Q, X, k, bits, also=None, ids=None, order=0, nthreads=16):
    """oracle.search_batch under the unpacked bits -> (labels [nq, k], dist [nq, k]), padded -1 / FLT_MAX"""
    X = np.asarray(X, np.float32)
    m = effective_mask(bits, X.shape[0], also)
    return oracle.search_batch(metric, np.asarray(Q, np.float32), X, k, order=order, mask=m, ids=ids, nthreads=nthreads)


def view_edge_counts(n, max_pct=MAX_PCT):
    """visible counts around the rule's edge, and one short of everything: (count, takes the row list)"""
    edge = n * max_pct // 100
    return [(c, rc.takes_row_list(c, n, max_pct)) for c in (edge - 1, edge, edge + 1, n - 1)]


def with_tail_ones(bits, n):
    """the same bitmap with every bit behind bit n - 1 of its last byte set: nothing of them may be read as a row"""
    out = np.array(bits, np.uint8, copy=True)
    if n & 7:
        out[-1] |= np.uint8((0xFF << (n & 7)) & 0xFF)
    return out


def block_gap_mask(n, rng):
    """rows in the first and the last block of BLOCK positions and none in the blocks between (n > 2 BLOCK)"""
    assert n > 2 * BLOCK
    m = np.zeros(n, np.uint8)
    m[rng.choice(BLOCK, 37, replace=False)] = 1
    last = (n - 1) // BLOCK * BLOCK
    m[last + rng.choice(n - last, min(5, n - last), replace=False)] = 1
    return m
