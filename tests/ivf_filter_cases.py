"""The row filter of the IVF-Flat index (include/longbow_gpu.h, lb_gpu_ivf_*: "filter") restated over tests/ivf_oracle.py, and
the masks tests/test_ivf_filter_semantics.py (CPU: the statement is pinned on them) and tests/test_gpu_ivf_filters.py (GPU) share.

The expected result needs no oracle of its own: a hidden row is a row in no list.  ivf_oracle.search with the hidden rows' lists
set to -1 probes the same lists (the probes come from the centroids alone), finds only visible rows in them (a probe is never
-1), and reports the visible rows it scanned per query."""
import numpy as np

from tests import code_filter_cases as cf
from tests import ivf_oracle as io
from tests import row_view_cases as rv

K = 10
LDS_KEYS = 16384                               # IVF_SELECT_LDS_KEYS
EDGE_COUNTS = (3, 130, 200, 300, 300, 600)     # rows per list of the tile-edge case
EDGE_KEEP = (0, 1, 127, 128, 129, 257)         # visible rows per list: around the scan's 128-row tile, and an emptied list


def search_filtered(oracle, metric, order, Q, X, C, lists, mask, k, nprobe, ids=None):
    """-> (labels [nq, k], dist [nq, k], visible rows scanned per query [nq])"""
    return io.search(oracle, metric, order, Q, X, C, np.where(np.asarray(mask) != 0, lists, -1), k, nprobe, ids=ids)


def parity_masks(n=3000, k=K, seed=31):
    """{name: mask} of code_filter_cases.masks over the rows of ivf_oracle.parity_case()"""
    return cf.masks(n, k, np.random.default_rng(seed))


def keep_per_list(lists, keep, rng=None):
    """0/1 mask that leaves list i exactly keep[i] rows: its first ones, or with rng a random choice of them"""
    lists = np.asarray(lists)
    m = np.zeros(lists.size, np.uint8)
    for l, cnt in enumerate(keep):
        rows = np.flatnonzero(lists == l)
        assert cnt <= rows.size, (l, cnt, rows.size)
        m[rows[:cnt] if rng is None else rows[np.flatnonzero(rv.exact_count_mask(rng, rows.size, cnt))]] = 1
    return m


def skew_mask(lists, keep0, seed=4):
    """list 0 keeps exactly keep0 rows, chosen at random; every other list stays whole"""
    sizes = np.bincount(lists)
    return keep_per_list(lists, [keep0] + sizes[1:].tolist(), np.random.default_rng(seed))
