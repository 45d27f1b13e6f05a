"""The list-major matrix-core tile of the IVF-SQ8 scan (kernels_ivfsq8_group.hip; the rule is stated at lb_gpu_ivfsq8_search):
labels, distance bits and last_search_stats against tests/ivfsq8_oracle.py (exact integers in numpy over the oracle's lists and
probes) at the shapes where the tile can go wrong, and lb_gpu_ivfsq8_last_route.  Every case that expects route 2 has
nq * nprobe >= 64 * nlist and every case that expects route 1 at most 2 pairs per list, so the assertions hold whatever the
measured threshold between them is (3 .. 64).  Bounds 0 / 255 make the scale exactly 1: integer-valued rows are their own codes."""
import numpy as np
import pytest

from tests import ivfsq8_oracle as sqo
from tests.gpu_util import assert_same
from tests.test_gpu_ivfsq8 import _check_search, _handle

pytestmark = pytest.mark.gpu
F = np.float32
K = 10
PAIR, TILE = 1, 2                        # lb_gpu_ivfsq8_last_route
EDGE_COUNTS = (0, 1, 127, 128, 129, 257)  # an empty list, the 128-row tile's edges, a third tile of one row


def _bounds(dims, hi=255):
    return np.zeros(dims, F), np.full(dims, hi, F)


def _edge(dims, nq=400):
    """centroids 60 + 100 e_i, list i of EDGE_COUNTS[i] rows (centroid + integer noise <= 20), shuffled -> X, Q, C, owner, ids"""
    rng = np.random.default_rng(9)
    nlist = len(EDGE_COUNTS)
    C_ = (F(60) + F(100) * np.eye(nlist, dims)).astype(F)
    owner = rng.permutation(np.repeat(np.arange(nlist), EDGE_COUNTS))
    X = (C_[owner] + rng.integers(-20, 21, (owner.size, dims))).astype(F)
    Q = (C_[rng.integers(0, nlist, nq)] + rng.integers(-20, 21, (nq, dims))).astype(F)
    return X, Q, C_, owner, np.arange(owner.size, dtype=np.int64) * 7 + 3


# 136: a stride of 144, two chunks, the second a single piece
@pytest.mark.parametrize("dims", [16, 136])
def test_tile_edges(oracle, dims):
    X, Q, C_, owner, ids = _edge(dims)
    mn, mx = _bounds(dims)
    lists, codes = sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)
    assert np.array_equal(lists, owner) and np.array_equal(codes, X.astype(np.uint8))
    h = _handle(X, C_, mn, mx, ids=ids)
    assert h.last_route() == 0  # no search yet
    for nprobe in (1, len(EDGE_COUNTS)):
        _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, K, nprobe, ids=ids, ctx=f"dims {dims} nprobe {nprobe}")
        assert h.last_route() == TILE, nprobe
    h.Close()


def _two_lists(oracle, X, Q, mn, mx, k=K):
    """two of the rows as centroids, every list probed -> labels, dist, the route"""
    C_ = X[[X.shape[0] // 3, 2 * X.shape[0] // 3]].copy()
    lists, codes = sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)
    h = _handle(X, C_, mn, mx)
    _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, k, 2, ctx=f"dims {X.shape[1]} nq {Q.shape[0]}")
    out = h.search(Q, k, 2) + (h.last_route(),)
    h.Close()
    return out


# 1: a padded stride; 20: a padded K-step; 80: a partial chunk; 768: six chunks; 8192: the largest S, 64 chunks
@pytest.mark.parametrize("dims", [1, 16, 20, 80, 768, 8192])
def test_dimensions(oracle, dims):
    rng = np.random.default_rng(dims)
    n, nq = 150, 64
    X, Q = rng.random((n, dims), dtype=F), rng.random((nq, dims), dtype=F)
    if dims == 8192:  # test_the_largest_s's rows and queries (tests/test_gpu_ivfsq8.py): codes all 0 against all 255
        X[17], X[120], Q[0], Q[1] = 0.0, 1.0, 1.0, 0.0
    lab, dist, route = _two_lists(oracle, X, Q, *_bounds(dims, 1), k=n if dims == 8192 else K)
    assert route == TILE
    if dims == 8192:
        assert lab[0, -1] == 17 and lab[1, -1] == 120 and dist[0, -1] == dist[1, -1] == F(8192 * 65025)
        assert lab[0, 0] == 120 and dist[0, 0] == 0.0


@pytest.mark.parametrize("dims", [16, 136])
@pytest.mark.parametrize("nq", [31, 32, 33, 64, 65, 127, 1030])
def test_group_edges_and_a_second_batch(oracle, nq, dims):
    """one column, its boundary, a full group, a second group of 1 and 63 pairs, two batches; below 64 the threshold decides"""
    rng = np.random.default_rng(dims + nq)
    X, Q = rng.integers(0, 256, (100, dims)).astype(F), rng.integers(0, 256, (nq, dims)).astype(F)
    route = _two_lists(oracle, X, Q, *_bounds(dims))[2]
    assert route == TILE if nq >= 64 else route in (PAIR, TILE)


def test_the_order_is_the_integers(oracle):
    """sqo.rounding_case: S = 2^24 + 1, 2^24, 2^24 + 1, 2^24, one float.  64 copies of its query are 128 pairs over 2 lists"""
    X, Q, C_, mn, mx = sqo.rounding_case()
    Q = np.repeat(Q, 64, axis=0)
    lists, codes = sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)
    h = _handle(X, C_, mn, mx)
    _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, 4, 2, ctx="rounding case")
    lab, dist = h.search(Q, 4, 2)
    assert h.last_route() == TILE
    assert (lab == np.array([1, 3, 0, 2])).all() and (dist == F(16777216.0)).all()
    h.Close()


@pytest.mark.parametrize("how", ["set_filter", "remove_rows", "bitmap"])
def test_filters_and_removals(oracle, how):
    from longbow_amd import ivfsq8
    X, Q, C_, owner, ids = _edge(136)
    mn, mx = _bounds(136)
    codes, nprobe = sqo.encode(X, mn, mx), len(EDGE_COUNTS)
    mask = (np.random.default_rng(3).random(X.shape[0]) < 0.6).astype(np.uint8)
    h = _handle(X, C_, mn, mx, ids=ids)
    if how == "set_filter":
        h.set_filter(mask)
    elif how == "remove_rows":
        assert h.remove_rows(np.flatnonzero(mask == 0)) == int((mask == 0).sum())
    bits = ivfsq8.pack_bitmap(mask)[0] if how == "bitmap" else None
    ol, od, scanned = sqo.search(oracle, 0, Q, C_, owner, codes, mn, mx, K, nprobe, ids=ids, mask=mask)
    lab, dist = h.search(Q, K, nprobe, bitmap=bits)
    assert_same(lab, dist, ol, od, how)
    assert h.last_search_stats() == (Q.shape[0], int(scanned.sum()), int(scanned.max()), Q.shape[0])
    assert how == "bitmap" or h.last_route() == TILE
    h.Close()


def test_the_per_pair_walk_stays_covered(oracle):
    """256 queries x 4 probes over 512 lists is 2 pairs a list: the per-pair scan, list 0 being three tiles of two chunks"""
    nlist, dims = 512, 136
    rng = np.random.default_rng(21)
    mn, mx = _bounds(dims)
    C_ = rng.integers(20, 236, (nlist, dims)).astype(F)
    owner = rng.permutation(np.repeat(np.arange(nlist), (300,) + (1,) * (nlist - 1)))
    X = (C_[owner] + rng.integers(-3, 4, (owner.size, dims))).astype(F)
    Q = (C_[rng.integers(0, 8, 256)] + rng.integers(-3, 4, (256, dims))).astype(F)
    lists, codes = sqo.assign(oracle, 0, X, C_), sqo.encode(X, mn, mx)
    assert np.bincount(lists, minlength=nlist)[0] == 300
    h = _handle(X, C_, mn, mx)
    _check_search(oracle, h, 0, Q, C_, lists, codes, mn, mx, K, 4, ctx="per pair")
    assert h.last_route() == PAIR
    h.Close()
