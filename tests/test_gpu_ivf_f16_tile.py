"""The list-major tile of the IVF-Flat float16 scan (kernels_ivf_f16_group.hip; the rule is stated at lb_gpu_ivf_search): labels
and distance bits against tests/ivf_oracle.py over the widened rows X16.astype(float32), at the shapes where the fp16 stage, the
grouping and the tile can go wrong, and lb_gpu_ivf_last_route.  Every case that expects route 2 has nq * nprobe >= 64 * nlist
and every case that expects route 1 at most 2 pairs per list or a shape the tile never takes, so the assertions hold whatever
the measured threshold between them is."""
import numpy as np
import pytest

from tests import ivf_filter_cases as fc
from tests import ivf_oracle as io
from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu
F, H = np.float32, np.float16
K = 10
PAIR, TILE = 1, 2                      # lb_gpu_ivf_last_route
EDGE_COUNTS = (0, 1, 63, 64, 65, 129)  # an empty list, the 64-row tile's edges, a second tile of one row


def _f16(X16, C_, metric=0, order=0, ids=None):
    from longbow_amd import ivf
    from longbow_amd.gpu import DataType
    gpu_or_skip()
    assert X16.dtype == H
    h = ivf.IVFFlat(C_, metric, order, dtype=DataType.Float16)
    h.add(X16, ids)
    return h


@pytest.fixture(scope="module")
def edge():
    """io.edge_case's lists of EDGE_COUNTS rows at 136 dimensions (the last chunk is one 16-byte piece) rounded to fp16, with ids,
    and 400 queries near the centroids"""
    X, _, C_, _ = io.edge_case(EDGE_COUNTS, dim=136)
    rng = np.random.default_rng(9)
    Q = (C_[rng.integers(0, len(EDGE_COUNTS), 400)] + rng.standard_normal((400, 136)).astype(F) * F(0.01)).astype(F)
    X16 = X.astype(H)
    return X16, X16.astype(F), Q, C_, np.arange(X.shape[0], dtype=np.int64) * 7 + 3


@pytest.mark.parametrize("metric,order", [(m, o) for m in (0, 1, 2) for o in (0, 1)])
def test_metrics_and_orders_at_the_tile_edges(oracle, edge, metric, order):
    X16, W, Q, C_, ids = edge
    lists = io.assign(oracle, metric, order, W, C_)
    h = _f16(X16, C_, metric, order, ids)
    assert np.array_equal(h.assignments(), lists)
    for nprobe, route in ((1, (PAIR, TILE)), (6, (TILE,))):
        lab, dist = h.search(Q, K, nprobe)
        assert h.last_route() in route, (nprobe, h.last_route())
        assert_same(lab, dist, *io.search(oracle, metric, order, Q, W, C_, lists, K, nprobe, ids=ids)[:2], f"metric {metric} order {order} nprobe {nprobe}")
    h.Close()


def _two_lists(oracle, dim, nq, n=150):
    X, Q, C_ = io.parity_case(n=n, dim=dim, nlist=2, nq=nq)
    X16 = X.astype(H)
    W = X16.astype(F)
    h = _f16(X16, C_)
    assert h.last_route() == 0  # no search yet
    lab, dist = h.search(Q, K, 2)
    assert_same(lab, dist, *io.search(oracle, 0, 0, Q, W, C_, io.assign(oracle, 0, 0, W, C_), K, 2)[:2], f"dim {dim} nq {nq}")
    route = h.last_route()
    h.Close()
    return route


@pytest.mark.parametrize("dim,route", [(8, TILE), (64, TILE), (72, TILE), (128, TILE), (136, TILE), (768, TILE), (12, PAIR), (4, PAIR)])
def test_dimensions(oracle, dim, route):
    """D % 8 != 0 takes the one-lane-per-row form even where the float32 handle would tile"""
    assert _two_lists(oracle, dim, 64) == route


@pytest.mark.parametrize("nq,route", [(17, (PAIR, TILE)), (33, (PAIR, TILE)), (64, (TILE,)), (65, (TILE,)), (127, (TILE,)), (1030, (TILE,))])
def test_group_edges_and_a_second_batch(oracle, nq, route):
    """every list is probed by every query: groups of 17 and 33 pairs (two and three query columns, one pair in the last), of 64,
    64 + 1 and 64 + 63 pairs; 1,030 queries are two batches"""
    assert _two_lists(oracle, 8, nq, n=100) in route


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_special_values_through_the_tile(metric):
    """+-inf, NaN, fp16 subnormals, +-65504 and +-0 in the rows: the float32 handle over the widened rows, NaN included"""
    from longbow_amd import ivf
    rng = np.random.default_rng(9)
    X16 = rng.standard_normal((300, 8)).astype(H)
    C_ = X16[[3, 100]].astype(F)
    X16[17, 4], X16[18, 0], X16[19], X16[20, 1] = np.nan, np.inf, 0.0, -np.inf
    X16[21], X16[22] = H(2.0 ** -24), H(2.0 ** -15)  # the smallest fp16 subnormal, half the smallest normal
    X16[23, 2], X16[23, 3], X16[24], X16[25, ::2] = H(65504.0), H(-65504.0), -0.0, H(-2.0 ** -24)
    Q = rng.standard_normal((64, 8)).astype(F)
    Q[3, 2] = np.nan
    Q[2] *= F(1.0e4)
    for order in (0, 1):
        h16, h32 = _f16(X16, C_, metric, order), ivf.IVFFlat(C_, metric, order)
        h32.add(X16.astype(F))
        (l16, d16), (l32, d32) = h16.search(Q, 300, 2), h32.search(Q, 300, 2)
        assert (h16.last_route(), h32.last_route()) == (TILE, TILE)
        assert np.array_equal(l16, l32) and np.array_equal(d16, d32, equal_nan=True), (metric, order)
        h16.Close()
        h32.Close()


@pytest.mark.parametrize("how", ["set_filter", "remove_rows", "bitmap"])
def test_filters_and_removals(oracle, edge, how):
    from longbow_amd import ivf
    X16, W, Q, C_, ids = edge
    lists = io.assign(oracle, 0, 0, W, C_)
    mask = (np.random.default_rng(3).random(X16.shape[0]) < 0.6).astype(np.uint8)
    h = _f16(X16, C_, ids=ids)
    if how == "set_filter":
        h.set_filter(mask)
    elif how == "remove_rows":
        assert h.remove_rows(np.flatnonzero(mask == 0)) == int((mask == 0).sum())
    bits = ivf.pack_bitmap(mask)[0] if how == "bitmap" else None
    lab, dist = h.search(Q, K, 6, bitmap=bits)
    assert_same(lab, dist, *fc.search_filtered(oracle, 0, 0, Q, W, C_, lists, mask, K, 6, ids=ids)[:2], how)
    assert how == "bitmap" or h.last_route() == TILE
    h.Close()


def test_the_per_pair_walk_stays_covered(oracle):
    """1,024 queries x 4 probes over 2,048 lists is 2 pairs a list: the per-pair scan, one workgroup walking list 0's three tiles
    of two chunks"""
    nlist, dim = 2048, 136
    rng = np.random.default_rng(21)
    C_ = (rng.standard_normal((nlist, dim)) * 10).astype(F)
    owner = rng.permutation(np.repeat(np.arange(nlist), (300,) + (1,) * (nlist - 1)))
    X16 = (C_[owner] + rng.standard_normal((owner.size, dim)).astype(F) * F(0.01)).astype(H)
    W = X16.astype(F)
    Q = (C_[rng.integers(0, 8, 1024)] + rng.standard_normal((1024, dim)).astype(F) * F(0.01)).astype(F)
    h = _f16(X16, C_)
    assert np.array_equal(h.assignments(), owner)
    lab, dist = h.search(Q, K, 4)
    assert h.last_route() == PAIR
    assert_same(lab, dist, *io.search(oracle, 0, 0, Q, W, C_, owner, K, 4)[:2])
    h.Close()
