"""Inputs of the IVF-Flat removal tests (tests/test_gpu_ivf_remove.py on the GPU, tests/test_ivf_remove_semantics.py on the CPU),
built from tests/ivf_oracle.py (parity_case, edge_case, skew_case), tests/ivf_filter_cases.py (keep_per_list) and
tests/remove_cases.py (fractions, ids, overlap sets).  Seeded, never written to.  Also same_handles, the comparison of a handle
with a fresh one of its survivors that the GPU file shares with tests/test_gpu_lifecycle.py.

The expected result needs no oracle of its own: a removed row is a row in no list.  ivf_oracle.search with the removed rows' lists
set to -1, as ivf_filter_cases.search_filtered does for hidden rows, probes the same lists (the probes come from the centroids
alone), finds only live rows in them, and reports the live rows it scanned per query."""
import functools

import numpy as np

from tests import ivf_filter_cases as fc
from tests import ivf_i8_oracle as o8
from tests import ivf_oracle as io
from tests import remove_cases as rc
from tests.gpu_util import assert_same

F = np.float32
NPROBES = (1, 4, 16)
KS = (1, 10, 100)
LDS_KEYS = fc.LDS_KEYS                                  # IVF_SELECT_LDS_KEYS
EDGE_COUNTS, EDGE_KEEP = fc.EDGE_COUNTS, fc.EDGE_KEEP   # rows per list, and the live rows each list is left
SKEW_KEEP = (LDS_KEYS + 1, LDS_KEYS, LDS_KEYS - 1)      # live rows of list 0, in the order one handle reaches them
FRACTIONS = rc.FRACTIONS
I8_SCALE = 30                                           # parity_case rows as int8 (tests/test_gpu_ivf_i8.py's scale)
live_mask, ids_for, overlap_sets, removed_rows, queries, filter_mask = (rc.live_mask, rc.ids_for, rc.overlap_sets, rc.removed_rows,
                                                                         rc.queries, rc.filter_mask)


def visible(live, mask=None):
    """rows a search can see: live, and under a filter visible too"""
    return (np.asarray(live) != 0) if mask is None else (np.asarray(live) != 0) & (np.asarray(mask) != 0)


def search_live(oracle, metric, order, Q, X, C, lists, live, k, nprobe, ids=None, mask=None):
    """-> (labels [nq, k], dist [nq, k], live and visible rows scanned per query [nq])"""
    return io.search(oracle, metric, order, Q, X, C, np.where(visible(live, mask), lists, -1), k, nprobe, ids=ids)


def search_live_i8(oracle, metric, order, Q8, X8, C, lists, live, k, nprobe, ids=None, mask=None):
    return o8.search(oracle, metric, order, Q8, X8, C, lists, k, nprobe, ids=ids, mask=visible(live, mask).astype(np.uint8))


def counts(h):
    return h.ntotal, h.nlive(), h.ndeleted()


def same_handles(h, fresh, Q, ctx, ks=KS, nprobes=NPROBES):
    """two IVF-Flat handles on a GPU answer alike: h (compacted) is what an add of the survivors (fresh) would have made"""
    assert counts(h) == counts(fresh) and h.nvisible() == fresh.nvisible(), ctx
    assert np.array_equal(h.assignments(), fresh.assignments()) and np.array_equal(h.list_sizes(), fresh.list_sizes()), ctx
    for nprobe in nprobes:
        for k in ks:
            assert_same(*h.search(Q, k, nprobe), *fresh.search(Q, k, nprobe), f"{ctx} nprobe {nprobe} k {k}")
            assert h.last_search_stats() == fresh.last_search_stats(), ctx


@functools.lru_cache(maxsize=None)
def parity(oracle, kind, metric):
    """parity_case for a handle of element type `kind` (f32 / f16 / i8), once per process -> (the handle's rows, its queries, its
    centroids, what the oracle reads as the rows, the oracle's lists of them at order 0).  float16: the rows rounded, the oracle
    reads them widened; int8: rows and queries scaled and rounded, the centroids scaled with them"""
    X, Q, C = io.parity_case()
    if kind == "i8":
        X, Q, C = o8.to_i8(X, I8_SCALE), o8.to_i8(Q, I8_SCALE), (C * F(I8_SCALE)).astype(F)
        out = (X, Q, C, X, o8.assign(oracle, metric, 0, X, C))
    elif kind == "f16":
        X16 = X.astype(np.float16)
        W = X16.astype(F)
        out = (X16, Q, C, W, io.assign(oracle, metric, 0, W, C))
    else:
        out = (X, Q, C, X, io.assign(oracle, metric, 0, X, C))
    for a in out:
        a.setflags(write=False)
    return out


def parity_lists(oracle, metric):
    """the oracle's lists of parity_case's f32 rows"""
    return parity(oracle, "f32", metric)[4]


def readback_sets(lists):
    """name -> removed rows of the read-back test; `one list`: every row of the longest list, which is emptied"""
    n = len(lists)
    out = dict(rc.readback_sets(n))
    out["one list"] = np.flatnonzero(np.asarray(lists) == np.argmax(np.bincount(lists)))
    return out


READBACK_NAMES = ("none", "first", "last", "every other", "one list", "all but one", "all")


def edge_removed(owner, rng=None):
    """the rows whose removal leaves list i exactly EDGE_KEEP[i] live rows: all but its first ones, or with rng a random choice"""
    return np.flatnonzero(fc.keep_per_list(owner, EDGE_KEEP, rng) == 0).astype(np.int64)


def edge_case_i8():
    """edge_case with noise wide enough to survive the rounding to int8: rows of a list differ, and stay nearest their centroid"""
    X, Q, C, owner = io.edge_case(EDGE_COUNTS, noise=3.0)
    return o8.to_i8(X, 1), o8.to_i8(Q, 1), C, owner


def skew_queries(Q):
    """skew_case's five queries and three more near centroid 0: eight"""
    return np.concatenate([Q, (Q[:3] * F(0.5)).astype(F)])


def skew_steps(lists):
    """[(live rows of list 0, rows to remove to get there from the step before)]: first down to SKEW_KEEP[0], a random choice, then
    one more row of list 0 at a time"""
    lists = np.asarray(lists)
    first = np.flatnonzero(fc.skew_mask(lists, SKEW_KEEP[0]) == 0).astype(np.int64)
    left = np.setdiff1d(np.flatnonzero(lists == 0), first)
    return [(SKEW_KEEP[0], first), (SKEW_KEEP[1], left[:1].astype(np.int64)), (SKEW_KEEP[2], left[1:2].astype(np.int64))]
