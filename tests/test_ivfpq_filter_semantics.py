"""tests/ivfpq_filter_cases.py's search_filtered against an independent statement of the filtered IVF-PQ search (the full ADC
ranking restricted to the probed and visible rows), and the conditions tests/test_gpu_ivfpq_filters.py relies on in its inputs,
asserted here on the CPU instead of assumed there."""
import numpy as np
import pytest

from tests import ivf_filter_cases as fc
from tests import ivf_oracle as io
from tests import ivfpq_filter_cases as pfc
from tests import ivfpq_oracle as pqo


@pytest.fixture(scope="module")
def parity(oracle):
    X, Q, C, cb = pqo.parity_case(*pqo.PARITY_SHAPES[0])
    lists, codes = pqo.assign(oracle, 0, X, C), pqo.encode(oracle, cb, X)
    full_l, full_d = pqo.brute(oracle, cb, Q, codes, X.shape[0])  # the whole ranking of every query, once
    return Q, C, cb, lists, codes, full_l, full_d


def test_search_filtered_is_the_full_ranking_restricted_to_the_probed_and_visible_rows(oracle, parity):
    Q, C, cb, lists, codes, full_l, full_d = parity
    masks = fc.parity_masks()
    assert len(masks) == 12
    differ = 0
    for nprobe in (3, C.shape[0]):
        probes = [io.probes(oracle, 0, 0, Q[j], C, nprobe) for j in range(Q.shape[0])]  # of the centroids alone: no mask plays a part
        plain_l, plain_d, _ = pqo.search(oracle, cb, 0, Q, C, lists, codes, pfc.K, nprobe)
        for name, mask in masks.items():
            lab, dist, scanned = pfc.search_filtered(oracle, cb, 0, Q, C, lists, codes, mask, pfc.K, nprobe)
            for j in range(Q.shape[0]):
                keep = np.isin(lists[full_l[j]], probes[j]) & (mask[full_l[j]] != 0)
                assert scanned[j] == keep.sum(), (name, nprobe, j)
                want_l, want_d = full_l[j][keep][:pfc.K], full_d[j][keep][:pfc.K]
                pad = pfc.K - want_l.size
                assert np.array_equal(lab[j], np.concatenate((want_l, np.full(pad, -1, np.int64)))), (name, nprobe, j)
                assert np.array_equal(dist[j], np.concatenate((want_d, np.full(pad, pqo.FLT_MAX, pqo.F)))), (name, nprobe, j)
            differ += int(not (np.array_equal(lab, plain_l) and np.array_equal(dist, plain_d)))
    assert differ > 0  # a search that ignored the filter would not pass the GPU parity test ...
    assert differ == 20  # ... under any mask but the two that hide none of the first K rows, at either nprobe


def test_edge_keeps(oracle):
    """what the GPU tile-edge case relies on: list i keeps exactly EDGE_KEEP_x[i] rows, first rows or a random choice, query i
    probes list i, and B's long visible list needs the scan's stride loop to take a second step"""
    X, Q, C, owner, cb = pqo.edge_case()
    assert np.bincount(owner, minlength=len(pqo.EDGE_COUNTS)).tolist() == list(pqo.EDGE_COUNTS)
    for keep in (pfc.EDGE_KEEP_A, pfc.EDGE_KEEP_B):
        assert len(keep) == len(pqo.EDGE_COUNTS) and all(k <= c for k, c in zip(keep, pqo.EDGE_COUNTS))
        first, rand = fc.keep_per_list(owner, keep), fc.keep_per_list(owner, keep, np.random.default_rng(6))
        for m in (first, rand):
            assert np.bincount(owner[m != 0], minlength=len(keep)).tolist() == list(keep)
        assert not np.array_equal(first, rand)
    assert pfc.EDGE_KEEP_A[2:6] == (pfc.TILE - 1, pfc.TILE - 1, pfc.TILE, pfc.TILE + 1) and pfc.EDGE_KEEP_A[:2] == (0, 0)
    assert pfc.EDGE_KEEP_B[pqo.EDGE_LONG] == 8193 == max(pfc.EDGE_KEEP_B)
    assert Q.shape[0] == 66 and pqo.scan_groups(66, 8193) == 8 and pqo.scan_groups(66, 8193) * pfc.TILE < 8193


def test_edge_keep_results(oracle):
    X, Q, C, owner, cb = pqo.edge_case()
    codes = pqo.encode(oracle, cb, X)
    mask = fc.keep_per_list(owner, pfc.EDGE_KEEP_A)
    nlist = C.shape[0]
    lab, dist, scanned = pfc.search_filtered(oracle, cb, 0, Q[:nlist], C, owner, codes, mask, pfc.K, 1)
    assert scanned.tolist() == list(pfc.EDGE_KEEP_A)
    assert (lab[1] == -1).all() and (dist[1] == pqo.FLT_MAX).all()  # list 1's one row is hidden: a probed list with no visible row
    assert lab[7, 0] == np.flatnonzero(owner == 7)[0] and (lab[7, 1:] == -1).all()


def test_skew_masks_straddle_the_lds_selection(oracle):
    X, Q, C, cb = pqo.skew_case()
    lists = pqo.assign(oracle, 0, X, C)
    for keep0 in (pfc.LDS_KEYS, pfc.LDS_KEYS + 1):
        m = fc.skew_mask(lists, keep0)
        vis = np.bincount(lists[m != 0], minlength=4)
        assert vis[0] == keep0 and vis[2] == np.count_nonzero(lists == 2) <= pfc.LDS_KEYS
