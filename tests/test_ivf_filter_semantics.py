"""tests/ivf_filter_cases.py's search_filtered against an independent statement of the filtered IVF-Flat search, and the
conditions tests/test_gpu_ivf_filters.py relies on in its inputs, asserted here on the CPU instead of assumed there."""
import numpy as np
import pytest

from tests import ivf_filter_cases as fc
from tests import ivf_oracle as io
from tests.gpu_util import oracle_topk_rows_parallel


@pytest.fixture(scope="module")
def parity(oracle):
    X, Q, C = io.parity_case()
    return X, Q, C, io.assign(oracle, 0, 0, X, C)


@pytest.mark.parametrize("name", list(fc.parity_masks()))
def test_search_filtered_is_the_knn_of_the_visible_rows_of_the_probed_lists(oracle, parity, name):
    X, Q, C, lists = parity
    mask = fc.parity_masks()[name]
    visible = mask != 0
    for nprobe in (1, 3, C.shape[0]):
        lab, dist, scanned = fc.search_filtered(oracle, 0, 0, Q, X, C, lists, mask, fc.K, nprobe)
        for j in range(Q.shape[0]):
            pr = io.probes(oracle, 0, 0, Q[j], C, nprobe)  # of the centroids alone: the mask plays no part
            rows = np.flatnonzero(visible & np.isin(lists, pr))
            wl, wd = oracle_topk_rows_parallel(oracle, 0, Q[j], X, fc.K, nthreads=4, visible=rows)
            assert np.array_equal(lab[j], wl) and np.array_equal(dist[j], wd), (name, nprobe, j)
            assert scanned[j] == rows.size
            if nprobe == C.shape[0]:  # every list probed: the k-NN of the visible rows
                fl, fd = oracle_topk_rows_parallel(oracle, 0, Q[j], X, fc.K, nthreads=4, visible=np.flatnonzero(mask))
                assert np.array_equal(lab[j], fl) and np.array_equal(dist[j], fd), (name, j)
                assert scanned[j] == np.count_nonzero(mask)


def test_the_masks_reach_the_edges(parity):
    X, Q, C, lists = parity
    masks = fc.parity_masks()
    assert masks["all-zero"].sum() == 0 and (masks["all-one"] == 1).all()
    assert {1, 2, 0x80, 0xFF} <= set(np.unique(masks["10 % byte mask"]).tolist())
    sizes = lambda m: np.bincount(lists[m != 0], minlength=C.shape[0])
    assert (sizes(masks["row 0"]) == 0).sum() == C.shape[0] - 1       # all lists but one become empty
    assert (sizes(masks["10 % byte mask"]) > 0).all() and (sizes(masks["10 % byte mask"]) < np.bincount(lists)).all()


def test_edge_case_shape(oracle):
    """list i keeps exactly EDGE_KEEP[i] of its EDGE_COUNTS[i] rows, first rows or a random choice, and query i probes list i"""
    X, Q, C, owner = io.edge_case(fc.EDGE_COUNTS)
    assert np.array_equal(io.assign(oracle, 0, 0, X, C), owner)
    assert [int(io.probes(oracle, 0, 0, Q[i], C, 1)[0]) for i in range(len(fc.EDGE_COUNTS))] == list(range(len(fc.EDGE_COUNTS)))
    first, rand = fc.keep_per_list(owner, fc.EDGE_KEEP), fc.keep_per_list(owner, fc.EDGE_KEEP, np.random.default_rng(6))
    for m in (first, rand):
        assert np.bincount(owner[m != 0], minlength=len(fc.EDGE_KEEP)).tolist() == list(fc.EDGE_KEEP)
    assert not np.array_equal(first, rand)
    lab, dist, scanned = fc.search_filtered(oracle, 0, 0, Q, X, C, owner, first, fc.K, 1)
    assert scanned.tolist() == list(fc.EDGE_KEEP)
    assert (lab[0] == -1).all() and (dist[0] == io.FLT_MAX).all()
    assert lab[1, 0] == np.flatnonzero(owner == 1)[0] and (lab[1, 1:] == -1).all()


def test_skew_masks_straddle_the_lds_selection(oracle):
    X, Q, C = io.skew_case()
    lists = io.assign(oracle, 0, 0, X, C)
    for keep0 in (fc.LDS_KEYS, fc.LDS_KEYS + 1):
        m = fc.skew_mask(lists, keep0)
        vis = np.bincount(lists[m != 0], minlength=4)
        assert vis[0] == keep0 and vis[2] == np.count_nonzero(lists == 2) <= fc.LDS_KEYS
        assert np.count_nonzero(lists == 0) > keep0 + 1000
