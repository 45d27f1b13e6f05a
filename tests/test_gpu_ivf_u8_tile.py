"""The list-major matrix-core tile of the IVF-Flat uint8 scan (kernels_ivf_u8_group.hip; the rule is stated at
lb_gpu_ivf_search): labels and distance bits against the numpy restatement of the reference's four chains (tests/test_gpu_u8.py)
over lists and probes from tests/ivf_oracle.py, at the shapes where the tile can go wrong, and lb_gpu_ivf_last_route.  Every case
that expects route 2 has nq * nprobe >= 64 * nlist and every case that expects route 1 at most 2 pairs per list (or a shape the
tile never takes), so the assertions hold whatever the measured threshold between them is."""
import numpy as np
import pytest

from tests import ivf_oracle as io
from tests.gpu_util import assert_same, gpu_or_skip
from tests.test_gpu_ivf_u8 import _chains, _draw
from tests.test_gpu_u8 import ref_dist, topk

pytestmark = pytest.mark.gpu
F, U8 = np.float32, np.uint8
K, EXACT = 10, 1 << 24
PAIR, TILE = 1, 2                        # lb_gpu_ivf_last_route
EDGE_COUNTS = (0, 1, 127, 128, 129, 257)  # an empty list, the 128-row tile's edges, a third tile of one row


def _handle(X, C_, ids=None):
    from longbow_amd import ivf
    gpu_or_skip()
    h = ivf.IVFFlatUint8(C_)
    h.add(X, ids)
    return h


def _want(oracle, Q, X, C_, lists, k, nprobe, ids=None, mask=None):
    D, seen = ref_dist(Q, X), np.ones(X.shape[0], bool) if mask is None else mask.astype(bool)
    out = []
    for j in range(Q.shape[0]):
        pr = np.arange(C_.shape[0]) if nprobe >= C_.shape[0] else io.probes(oracle, 0, 0, Q[j].astype(F), C_, nprobe)
        rows = io.probed_rows(lists, pr)
        rows = rows[seen[rows]]
        lab, dist = topk(D[j, rows], k, rows)
        out.append((np.where(lab < 0, lab, lab if ids is None else ids[np.maximum(lab, 0)]), dist))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _edge(dim, nq=400):
    """centroids 60 + 100 e_i, list i of EDGE_COUNTS[i] rows (its centroid plus integer noise of up to 20), shuffled, with ids;
    nq queries near the centroids"""
    rng = np.random.default_rng(9)
    nlist = len(EDGE_COUNTS)
    C_ = (F(60) + F(100) * np.eye(nlist, dim)).astype(F)
    owner = rng.permutation(np.repeat(np.arange(nlist), EDGE_COUNTS))
    X = (C_[owner] + rng.integers(-20, 21, (owner.size, dim))).astype(U8)
    Q = (C_[rng.integers(0, nlist, nq)] + rng.integers(-20, 21, (nq, dim))).astype(U8)
    return X, Q, C_, owner, np.arange(owner.size, dtype=np.int64) * 7 + 3


# 144: the totals form, the second stage a padded half K-step; 272: the chains form, a last chunk of one piece
@pytest.mark.parametrize("dim", [144, 272])
def test_tile_edges(oracle, dim):
    X, Q, C_, owner, ids = _edge(dim)
    lists = io.assign(oracle, 0, 0, X.astype(F), C_)
    assert np.array_equal(lists, owner)
    h = _handle(X, C_, ids)
    assert h.last_route() == 0  # no search yet
    for nprobe in (1, len(EDGE_COUNTS)):
        lab, dist = h.search(Q, K, nprobe)
        assert h.last_route() == TILE, (nprobe, h.last_route())
        assert_same(lab, dist, *_want(oracle, Q, X, C_, lists, K, nprobe, ids), f"dim {dim} nprobe {nprobe}")
    h.Close()


def _two_lists(oracle, X, Q, C_, misaligned=False):
    """every list probed; -> the route"""
    lists = io.assign(oracle, 0, 0, X.astype(F), C_)
    h = _handle(X, C_)
    if misaligned:  # queries at an odd byte address
        import torch
        nq = Q.shape[0]
        buf = torch.zeros(Q.size + 16, dtype=torch.uint8, device="cuda")
        buf[1:1 + Q.size] = torch.from_numpy(Q).cuda().reshape(-1)
        dD, dL = torch.full((nq, K), -5.0, device="cuda"), torch.full((nq, K), -5, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert buf.data_ptr() % 16 == 0
        h.search_device(nq, buf.data_ptr() + 1, K, 2, dD.data_ptr(), dL.data_ptr())
        lab, dist = dL.cpu().numpy(), dD.cpu().numpy()
    else:
        lab, dist = h.search(Q, K, 2)
    assert_same(lab, dist, *_want(oracle, Q, X, C_, lists, K, 2), f"dim {X.shape[1]} nq {Q.shape[0]}")
    route = h.last_route()
    h.Close()
    return route


@pytest.mark.parametrize("dim,data,route", [
    (16, "uniform", TILE), (32, "uniform", TILE), (128, "uniform", TILE), (256, "uniform", TILE),  # totals
    (272, "uniform", TILE), (768, "uniform", TILE),                                                # chains
    (768, "extremes", TILE), (1040, "extremes", TILE),  # every total above 2^24, no chain: the per-chain value decides
    (2048, "fallback", TILE),                           # chains above 2^24 beside chains below, in one tile
    (20, "uniform", PAIR), (100, "uniform", PAIR),      # one lane per row
    (16, "misaligned", PAIR)])
def test_dimensions_and_forms(oracle, dim, data, route):
    rng = np.random.default_rng(dim + len(data))
    n, nq = 150, 64
    if data == "fallback":  # rows in 0..20 against queries in 235..255, every second row near a query
        X, Q = rng.integers(0, 21, (n, dim)).astype(U8), rng.integers(235, 256, (nq, dim)).astype(U8)
        X[1::2] = np.clip(Q[rng.integers(0, nq, n // 2)].astype(np.int64) + rng.integers(-40, 41, (n // 2, dim)), 0, 255).astype(U8)
        S = _chains(Q, X)[0]
        assert S[:, :, 0::2].min() > EXACT and S[:, :, 1::2].max() <= EXACT
        # 128 +- 1 with as many of either sign: a row's list follows its own noise, so near and far rows share the lists
        C_ = np.stack([128 + rng.permutation(np.repeat([-1.0, 1.0], dim // 2)) for _ in range(2)]).astype(F)
    else:
        kind = "extremes" if data == "extremes" else "uniform"
        X, Q = _draw(rng, kind, n, dim), _draw(rng, kind, nq, dim)
        C_ = X[[n // 3, 2 * n // 3]].astype(F)
    if data == "extremes":
        (S, per_chain), D = _chains(Q, X), ref_dist(Q, X)
        assert S.sum(axis=0).min() > EXACT and S.max() <= EXACT and np.array_equal(per_chain, D)
        assert (D != np.sqrt(S.sum(axis=0).astype(F).astype(np.float64)).astype(F)).any()
    assert _two_lists(oracle, X, Q, C_, data == "misaligned") == route


@pytest.mark.parametrize("dim", [16, 272])
@pytest.mark.parametrize("nq", [31, 32, 33, 64, 65, 127, 1030])
def test_group_edges_and_a_second_batch(oracle, nq, dim):
    """every list is probed by every query: one column, the column boundary, one full group, a second group of 1 and of 63 pairs
    (the chains form splits every group by column); 1,030 queries are two batches.  Below 64 pairs a list the route is the
    measured threshold's to decide"""
    rng = np.random.default_rng(dim + nq)
    X, Q = _draw(rng, "uniform", 100, dim), _draw(rng, "uniform", nq, dim)
    route = _two_lists(oracle, X, Q, X[[33, 66]].astype(F))
    assert route == TILE if nq >= 64 else route in (PAIR, TILE)


@pytest.mark.parametrize("how", ["set_filter", "remove_rows", "bitmap"])
def test_filters_and_removals(oracle, how):
    from longbow_amd import ivf
    X, Q, C_, owner, ids = _edge(272)
    mask = (np.random.default_rng(3).random(X.shape[0]) < 0.6).astype(np.uint8)
    h = _handle(X, C_, ids)
    if how == "set_filter":
        h.set_filter(mask)
    elif how == "remove_rows":
        assert h.remove_rows(np.flatnonzero(mask == 0)) == int((mask == 0).sum())
    bits = ivf.pack_bitmap(mask)[0] if how == "bitmap" else None
    lab, dist = h.search(Q, K, len(EDGE_COUNTS), bitmap=bits)
    assert_same(lab, dist, *_want(oracle, Q, X, C_, owner, K, len(EDGE_COUNTS), ids, mask), how)
    assert how == "bitmap" or h.last_route() == TILE
    h.Close()


def test_the_per_pair_staged_walk_stays_covered(oracle):
    """256 queries x 4 probes over 512 lists is 2 pairs a list: the per-pair staged scan, one workgroup walking list 0's three
    tiles of two stages (272 dimensions, the chains form)"""
    nlist, dim = 512, 272
    rng = np.random.default_rng(21)
    C_ = rng.integers(20, 236, (nlist, dim)).astype(F)
    owner = rng.permutation(np.repeat(np.arange(nlist), (300,) + (1,) * (nlist - 1)))
    X = (C_[owner] + rng.integers(-3, 4, (owner.size, dim))).astype(U8)
    Q = (C_[rng.integers(0, 8, 256)] + rng.integers(-3, 4, (256, dim))).astype(U8)
    lists = io.assign(oracle, 0, 0, X.astype(F), C_)
    assert np.bincount(lists, minlength=nlist)[0] == 300
    h = _handle(X, C_)
    lab, dist = h.search(Q, K, 4)
    assert h.last_route() == PAIR
    assert_same(lab, dist, *_want(oracle, Q, X, C_, lists, K, 4))
    h.Close()
