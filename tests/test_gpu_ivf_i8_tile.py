"""The list-major i8 matrix-core tile of the IVF-Flat int8 scan (kernels_ivf_i8_group.hip; the rule is stated at
lb_gpu_ivf_search): labels and distance bits against tests/ivf_i8_oracle.py at the shapes where the tile can go wrong, and
lb_gpu_ivf_last_route.  Every case that expects route 2 has nq * nprobe >= 64 * nlist and every case that expects route 1 at
most 2 pairs per list (or a shape the tile never takes), so the assertions hold whatever the measured threshold between them is.
Lists always come from o8.assign."""
import numpy as np
import pytest

from tests import ivf_i8_oracle as o8
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F, B = np.float32, np.int8
K = 10
PAIR, TILE = 1, 2                        # lb_gpu_ivf_last_route
EDGE_COUNTS = (0, 1, 127, 128, 129, 257)  # an empty list, the 128-row tile's edges, a third tile of one row


def _handle(X8, C_, metric=0, ids=None):
    from longbow_amd import ivf
    gpu_or_skip()
    h = ivf.IVFFlatInt8(C_, metric)
    h.add(X8, ids)
    return h


def _edge(nq=400, dim=144):
    """centroids 100 e_i, list i of EDGE_COUNTS[i] rows (its centroid plus integer noise of up to 20), shuffled, with ids; nq
    queries near the centroids.  144 dimensions are two stages, the second a half K-step padded with zeros"""
    rng = np.random.default_rng(9)
    nlist = len(EDGE_COUNTS)
    C_ = (F(100) * np.eye(nlist, dim)).astype(F)
    owner = rng.permutation(np.repeat(np.arange(nlist), EDGE_COUNTS))
    X8 = (C_[owner] + rng.integers(-20, 21, (owner.size, dim))).astype(B)
    Q8 = (C_[rng.integers(0, nlist, nq)] + rng.integers(-20, 21, (nq, dim))).astype(B)
    return X8, Q8, C_, owner, np.arange(owner.size, dtype=np.int64) * 7 + 3


@pytest.mark.parametrize("metric", [0, 2])
def test_metrics_at_the_tile_edges(oracle, metric):
    X8, Q8, C_, owner, ids = _edge()
    lists = o8.assign(oracle, metric, 0, X8, C_)
    assert np.array_equal(lists, owner)
    h = _handle(X8, C_, metric, ids)
    assert h.last_route() == 0  # no search yet
    for nprobe, route in ((1, (PAIR, TILE)), (len(EDGE_COUNTS), (TILE,))):
        lab, dist = h.search(Q8, K, nprobe)
        assert h.last_route() in route, (nprobe, h.last_route())
        assert_same(lab, dist, *o8.search(oracle, metric, 0, Q8, X8, C_, lists, K, nprobe, ids=ids)[:2], f"metric {metric} nprobe {nprobe}")
    h.Close()


def _two_lists(oracle, dim, nq, metric=0, n=150, extreme=False):
    """full-range random rows and queries (extreme: drawn from {-128, 127}), two of the rows as centroids, every list probed"""
    rng = np.random.default_rng(dim + nq)
    draw = (lambda s: rng.choice(np.array([-128, 127], B), s)) if extreme else (lambda s: rng.integers(-128, 128, s).astype(B))
    X8, Q8 = draw((n, dim)), draw((nq, dim))
    C_ = X8[[n // 3, 2 * n // 3]].astype(F)
    lists = o8.assign(oracle, metric, 0, X8, C_)
    h = _handle(X8, C_, metric)
    lab, dist = h.search(Q8, K, 2)
    assert_same(lab, dist, *o8.search(oracle, metric, 0, Q8, X8, C_, lists, K, 2)[:2], f"dim {dim} nq {nq} metric {metric}")
    route = h.last_route()
    h.Close()
    return route


@pytest.mark.parametrize("dim,metric,extreme,route", [
    (16, 0, False, TILE), (32, 0, False, TILE), (128, 0, False, TILE), (144, 0, False, TILE), (768, 0, False, TILE),
    (1024, 2, False, TILE),
    (2048, 0, True, TILE),    # S passes 2^24: the single rounding
    (24, 0, False, PAIR),     # one lane per row
    (1040, 2, False, PAIR)])  # dot beyond 1,024 dimensions: one lane per row
def test_dimensions(oracle, dim, metric, extreme, route):
    assert _two_lists(oracle, dim, 64, metric, extreme=extreme) == route


@pytest.mark.parametrize("nq", [31, 32, 33, 64, 65, 127, 1030])
def test_group_edges_and_a_second_batch(oracle, nq):
    """every list is probed by every query: one column, the column boundary, one full group, a second group of 1 and of 63 pairs;
    1,030 queries are two batches.  Below 64 pairs a list the route is the measured threshold's to decide"""
    route = _two_lists(oracle, 16, nq, n=100)
    assert route == TILE if nq >= 64 else route in (PAIR, TILE)


@pytest.mark.parametrize("how", ["set_filter", "remove_rows", "bitmap"])
def test_filters_and_removals(oracle, how):
    from longbow_amd import ivf
    X8, Q8, C_, owner, ids = _edge()
    mask = (np.random.default_rng(3).random(X8.shape[0]) < 0.6).astype(np.uint8)
    h = _handle(X8, C_, ids=ids)
    if how == "set_filter":
        h.set_filter(mask)
    elif how == "remove_rows":
        assert h.remove_rows(np.flatnonzero(mask == 0)) == int((mask == 0).sum())
    bits = ivf.pack_bitmap(mask)[0] if how == "bitmap" else None
    lab, dist = h.search(Q8, K, len(EDGE_COUNTS), bitmap=bits)
    assert_same(lab, dist, *o8.search(oracle, 0, 0, Q8, X8, C_, o8.assign(oracle, 0, 0, X8, C_), K, len(EDGE_COUNTS), ids=ids, mask=mask)[:2], how)
    assert how == "bitmap" or h.last_route() == TILE
    h.Close()


def test_the_per_pair_staged_walk_stays_covered(oracle):
    """256 queries x 4 probes over 512 lists is 2 pairs a list: the per-pair staged scan, one workgroup walking list 0's three
    tiles of two stages (272 dimensions)"""
    nlist, dim = 512, 272
    rng = np.random.default_rng(21)
    C_ = rng.integers(-100, 101, (nlist, dim)).astype(F)
    owner = rng.permutation(np.repeat(np.arange(nlist), (300,) + (1,) * (nlist - 1)))
    X8 = (C_[owner] + rng.integers(-3, 4, (owner.size, dim))).astype(B)
    Q8 = (C_[rng.integers(0, 8, 256)] + rng.integers(-3, 4, (256, dim))).astype(B)
    lists = o8.assign(oracle, 0, 0, X8, C_)
    assert np.bincount(lists, minlength=nlist)[0] == 300
    h = _handle(X8, C_)
    lab, dist = h.search(Q8, K, 4)
    assert h.last_route() == PAIR
    assert_same(lab, dist, *o8.search(oracle, 0, 0, Q8, X8, C_, lists, K, 4)[:2])
    h.Close()
