"""The list-major tile of the IVF-Flat float32 scan (kernels_ivf_group.hip; the rule is stated at lb_gpu_ivf_search): labels and
distance bits against tests/ivf_oracle.py at the shapes where the grouping and the tile can go wrong, and lb_gpu_ivf_last_route.
Every case that expects route 2 has nq * nprobe >= 64 * nlist and every case that expects route 1 at most 2 pairs per list, so
the assertions hold whatever the measured threshold between them is."""
import numpy as np
import pytest

from tests import ivf_filter_cases as fc
from tests import ivf_oracle as io
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
K = 10
PAIR, TILE = 1, 2                      # lb_gpu_ivf_last_route
EDGE_COUNTS = (0, 1, 63, 64, 65, 129)  # an empty list, the 64-row tile's edges, a second tile of one row


def _handle(X, C_, metric=0, order=0, ids=None):
    from longbow_amd import ivf
    gpu_or_skip()
    h = ivf.IVFFlat(C_, metric, order)
    h.add(X, ids)
    return h


def _edge(nq=400, dim=68):
    """io.edge_case's lists of EDGE_COUNTS rows (two chunks, the second of four elements) with ids, and nq queries near the centroids"""
    X, _, C_, owner = io.edge_case(EDGE_COUNTS, dim=dim)
    rng = np.random.default_rng(9)
    Q = (C_[rng.integers(0, len(EDGE_COUNTS), nq)] + rng.standard_normal((nq, dim)).astype(F) * F(0.01)).astype(F)
    return X, Q, C_, owner, np.arange(X.shape[0], dtype=np.int64) * 7 + 3


@pytest.mark.parametrize("metric,order", [(m, o) for m in (0, 1, 2) for o in (0, 1)])
def test_metrics_and_orders_at_the_tile_edges(oracle, metric, order):
    X, Q, C_, owner, ids = _edge()
    h = _handle(X, C_, metric, order, ids)
    assert np.array_equal(h.assignments(), owner)
    for nprobe, route in ((1, (PAIR, TILE)), (6, (TILE,))):
        lab, dist = h.search(Q, K, nprobe)
        assert h.last_route() in route, (nprobe, h.last_route())
        assert_same(lab, dist, *io.search(oracle, metric, order, Q, X, C_, owner, K, nprobe, ids=ids)[:2], f"metric {metric} order {order} nprobe {nprobe}")
    h.Close()


def _two_lists(oracle, dim, nq, n=150):
    X, Q, C_ = io.parity_case(n=n, dim=dim, nlist=2, nq=nq)
    h = _handle(X, C_)
    assert h.last_route() == 0  # no search yet
    lab, dist = h.search(Q, K, 2)
    assert_same(lab, dist, *io.search(oracle, 0, 0, Q, X, C_, io.assign(oracle, 0, 0, X, C_), K, 2)[:2], f"dim {dim} nq {nq}")
    route = h.last_route()
    h.Close()
    return route


@pytest.mark.parametrize("dim,route", [(4, TILE), (64, TILE), (132, TILE), (768, TILE), (6, PAIR)])
def test_dimensions(oracle, dim, route):
    assert _two_lists(oracle, dim, 64) == route


@pytest.mark.parametrize("nq", [64, 65, 127, 1030])
def test_group_edges_and_a_second_batch(oracle, nq):
    """every list is probed by every query: groups of 64, 64 + 1 and 64 + 63 pairs; 1,030 queries are two batches"""
    assert _two_lists(oracle, 4 if nq == 1030 else 8, nq, n=100) == TILE


@pytest.mark.parametrize("how", ["set_filter", "remove_rows", "bitmap"])
def test_filters_and_removals(oracle, how):
    from longbow_amd import ivf
    X, Q, C_, owner, ids = _edge()
    mask = (np.random.default_rng(3).random(X.shape[0]) < 0.6).astype(np.uint8)
    h = _handle(X, C_, ids=ids)
    if how == "set_filter":
        h.set_filter(mask)
    elif how == "remove_rows":
        assert h.remove_rows(np.flatnonzero(mask == 0)) == int((mask == 0).sum())
    bits = ivf.pack_bitmap(mask)[0] if how == "bitmap" else None
    lab, dist = h.search(Q, K, 6, bitmap=bits)
    assert_same(lab, dist, *fc.search_filtered(oracle, 0, 0, Q, X, C_, owner, mask, K, 6, ids=ids)[:2], how)
    assert how == "bitmap" or h.last_route() == TILE
    h.Close()


def test_the_per_pair_walk_stays_covered(oracle):
    """1,024 queries x 4 probes over 2,048 lists is 2 pairs a list: the per-pair scan, one workgroup walking list 0's three tiles
    of three chunks"""
    nlist, dim = 2048, 136
    rng = np.random.default_rng(21)
    C_ = (rng.standard_normal((nlist, dim)) * 10).astype(F)
    owner = rng.permutation(np.repeat(np.arange(nlist), (300,) + (1,) * (nlist - 1)))
    X = (C_[owner] + rng.standard_normal((owner.size, dim)).astype(F) * F(0.01)).astype(F)
    Q = (C_[rng.integers(0, 8, 1024)] + rng.standard_normal((1024, dim)).astype(F) * F(0.01)).astype(F)
    h = _handle(X, C_)
    assert np.array_equal(h.assignments(), owner)
    lab, dist = h.search(Q, K, 4)
    assert h.last_route() == PAIR
    assert_same(lab, dist, *io.search(oracle, 0, 0, Q, X, C_, owner, K, 4)[:2])
    h.Close()
