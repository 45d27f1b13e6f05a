"""The row bitmap given with a search call on the IVF-PQ handle, plain ("pq") and residual ("rpq"), and on the IVF-SQ8 handle ("sq8")
(include/longbow_gpu.h: lb_gpu_ivfpq_search_bitmap_ctx, lb_gpu_ivfsq8_search_bitmap_ctx) restated for the tests
tests/test_ivf_code_bitmap_semantics.py (CPU: the statement is pinned here) and tests/test_gpu_ivf_code_bitmap.py (GPU) share.

Nothing here is new arithmetic.  The inputs are tests/ivf_code_remove_cases.py's Kinds and Cases, the bits tests/ivf_bitmap_cases.py's,
the masks tests/ivf_filter_cases.py's; the expected result of a search under a bitmap is the Kind's oracle with
mask = bits & filter & live, and with a stride one such search per query."""
import functools

import numpy as np

from tests import ivf_bitmap_cases as bc
from tests import ivf_code_remove_cases as cc
from tests import ivf_oracle as io
from tests import ivfpq_oracle as pqo
from tests import sq8_oracle as so

F = np.float32
K = 10


def search_bitmap(oracle, c, Q, bits, k, nprobe, also=None, ids=None, rows=None):
    """the oracle of the case's kind under the unpacked bits (ANDed with the 0/1 mask `also`: the handle's filter, liveness) over
    rows `rows` of the case (None: all) -> (labels, dist, rows scanned per query)"""
    n = c.n if rows is None else len(rows)
    m = bc.unpack(bits, n)
    if also is not None:
        m = m & (np.asarray(also) != 0)
    return c.search(oracle, Q, m, k, nprobe, ids=ids, rows=rows)


def search_strided(oracle, c, Q, bits2d, k, nprobe):
    """query q under bits2d[q]: one single-bitmap search per query"""
    labels = np.empty((Q.shape[0], k), np.int64)
    dist = np.empty((Q.shape[0], k), F)
    scanned = np.empty(Q.shape[0], np.int64)
    for q in range(Q.shape[0]):
        l, d, s = search_bitmap(oracle, c, Q[q:q + 1], bits2d[q], k, nprobe)
        labels[q], dist[q], scanned[q] = l[0], d[0], s[0]
    return labels, dist, scanned


@functools.lru_cache(maxsize=None)
def step_case(oracle, kind):
    """ivf_oracle.edge_case over ivf_bitmap_cases.STEP_COUNTS (16,388 rows in lists of 3, 2,047, 2,048, 2,049, 4,097 and 6,144: around
    the 2,048 list positions a workgroup of the compaction takes per step) with unit noise, so that the codes of a list differ, and
    the kind's codebooks or trained bounds; query i probes list i first"""
    X, Q, C, owner = io.edge_case(bc.STEP_COUNTS, dim=16, seed=5, noise=1.0)
    par = tuple(so.train(X)) if kind == "sq8" else pqo.codebooks(16, 4, 99)
    return cc.Case(oracle, kind, X, Q, C, par, lists=owner)


def shared_form(sizes, nq, nprobe, stride):
    """the host's rule (lb_ivf_host.h, ivf_search): under ONE bitmap, a call whose nq * pmax exceeds the rows its lists hold compacts
    every list once; otherwise, and under a bitmap per query, every (query, probe slot) compacts its list for itself.  sizes: of the
    lists the handle walks, the visible ones under its own filter or removals; pmax: the rows of the nprobe largest"""
    sizes = np.sort(np.asarray(sizes, np.int64))[::-1]
    pmax = max(int(sizes[:min(nprobe, sizes.size)].sum()), 1)
    return stride == 0 and nq * pmax > int(sizes.sum())
