"""The row filter of the IVF-PQ index (include/longbow_gpu.h, lb_gpu_ivfpq_*: "filter") restated over tests/ivfpq_oracle.py, and
the keeps tests/test_ivfpq_filter_semantics.py (CPU: the statement is pinned on them) and tests/test_gpu_ivfpq_filters.py (GPU)
share.  The masks are tests/ivf_filter_cases.py's.

As on the IVF-Flat index the expected result needs no oracle of its own: a hidden row is a row in no list.  ivfpq_oracle.search
with the hidden rows' lists set to -1 probes the same lists (the probes come from the centroids alone), finds only visible rows in
them (a probe is never -1), and reports the visible rows it scanned per query."""
import numpy as np

from tests import ivfpq_oracle as pqo

K = 10
LDS_KEYS = 16384  # IVF_SELECT_LDS_KEYS
TILE = pqo.TILE

# visible rows per list of ivfpq_oracle.edge_case(), whose lists hold (0, 1, 1023, 1024, 1025, 8269, 3, 5, 2, 0, 7) rows
# A: emptied lists, and visible lengths TILE - 1, TILE and TILE + 1, the last thinned from the long run
EDGE_KEEP_A = (0, 0, TILE - 1, TILE - 1, TILE, TILE + 1, 3, 1, 0, 0, 7)
# B: 8193 visible in the long list: at edge_case()'s 66 queries the scan has 8 workgroups a query, 8 * TILE < 8193, and the stride
# loop takes a second step
EDGE_KEEP_B = (0, 1, 0, TILE, TILE + 1, 8 * TILE + 1, 2, 5, 1, 0, 0)


def search_filtered(oracle, cb, order, Q, C, lists, codes, mask, k, nprobe, ids=None):
    """-> (labels [nq, k], dist [nq, k], visible rows scanned per query [nq])"""
    return pqo.search(oracle, cb, order, Q, C, np.where(np.asarray(mask) != 0, lists, -1), codes, k, nprobe, ids=ids)
