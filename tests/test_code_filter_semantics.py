"""What a filtered search over BQ or SQ8 codes must return, pinned on the CPU before the GPU is asked: the oracle on the visible
subset (tests/code_filter_cases.py: subset_search, the expected result of tests/test_gpu_code_filters.py) agrees with an
independent statement, the full distance matrix with the hidden rows at +inf and a stable argsort by (distance, row)."""
import numpy as np
import pytest

from tests import code_filter_cases as cf

CASES = [("bq", d) for d in cf.BQ_DIMS] + [("sq8", d) for d in cf.SQ8_DIMS]


@pytest.mark.parametrize("k", cf.KS)
@pytest.mark.parametrize("kind,dims", CASES)
def test_subset_oracle_equals_the_masked_matrix_statement(kind, dims, k):
    rng = np.random.default_rng(dims * 31 + k)
    n, nq = cf.N, 5
    codes = cf.codes_of(kind, rng, n, dims)
    q = cf.codes_of(kind, rng, nq, dims)
    q[0] = codes[n // 2]  # a query with a row at distance 0
    D = cf.dist_matrix(kind, q, codes)
    for name, mask in cf.masks(n, k, rng).items():
        vis = np.flatnonzero(mask)
        lab, dist = cf.subset_search(kind, q, codes, mask, k)
        wlab, wdist = cf.masked_topk(D, mask, k)
        assert np.array_equal(lab, wlab) and np.array_equal(dist, wdist), (name, kind, dims, k)
        have = min(k, vis.size)  # the visible rows first, then padding; labels are corpus rows
        assert (lab[:, have:] == -1).all() and (dist[:, have:] == cf.FLT_MAX).all(), name
        assert np.isin(lab[:, :have], vis).all() and (dist[:, :have] < cf.FLT_MAX).all(), name


def test_mask_bytes_other_than_one_are_visible():
    mask = np.array([0, 1, 2, 0x80, 0xFF, 0], np.uint8)
    codes = np.arange(6, dtype=np.uint64).reshape(6, 1)
    lab, _ = cf.subset_search("bq", codes[:1], codes, mask, 6)
    assert sorted(lab[0][lab[0] >= 0].tolist()) == [1, 2, 3, 4]
    assert np.array_equal(lab, cf.masked_topk(cf.dist_matrix("bq", codes[:1], codes), mask, 6)[0])


def test_ties_go_to_the_lowest_visible_rows():
    rng = np.random.default_rng(5)
    n, k = 1000, 7
    for kind, dims in (("bq", 64), ("sq8", 16)):
        codes = np.repeat(cf.codes_of(kind, rng, 1, dims), n, axis=0)
        mask = cf.rv.byte_mask(rng, n, 0.5)
        lab, dist = cf.subset_search(kind, codes[:1], codes, mask, k)
        assert np.array_equal(lab[0], np.flatnonzero(mask)[:k]) and (dist == 0).all()
        assert np.array_equal(lab, cf.masked_topk(cf.dist_matrix(kind, codes[:1], codes), mask, k)[0])
