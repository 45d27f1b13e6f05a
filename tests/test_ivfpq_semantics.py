"""tests/ivfpq_oracle.py against the brute-force ADC ranking, and the conditions tests/test_gpu_ivfpq.py relies on in its inputs,
asserted here on the CPU instead of assumed there."""
import numpy as np
import pytest

from tests import ivf_oracle as io
from tests import ivfpq_oracle as pqo


@pytest.mark.parametrize("dims,M", pqo.PARITY_SHAPES)
@pytest.mark.parametrize("order", [0, 1])
def test_every_list_probed_is_the_brute_adc_topk(oracle, dims, M, order):
    X, Q, C, cb = pqo.parity_case(dims, M, n=600, nq=5)
    lists, codes = pqo.assign(oracle, order, X, C), pqo.encode(oracle, cb, X)
    bl, bd = pqo.brute(oracle, cb, Q, codes, 10)
    for j in range(Q.shape[0]):  # brute is the flat ranking of adc_batch over every code
        oi, od, _ = oracle.topk_canonical(oracle.adc_batch(oracle.build_adc_table(cb, Q[j]), codes), 10)
        assert np.array_equal(bl[j], oi) and np.array_equal(bd[j], od)
    for nprobe in (C.shape[0], C.shape[0] + 5):
        lab, dist, scanned = pqo.search(oracle, cb, order, Q, C, lists, codes, 10, nprobe)
        assert np.array_equal(lab, bl) and np.array_equal(dist, bd)
        assert (scanned == X.shape[0]).all()


@pytest.mark.parametrize("dims,M", pqo.PARITY_SHAPES)
def test_result_is_the_brute_ranking_restricted_to_the_probed_rows(oracle, dims, M):
    X, Q, C, cb = pqo.parity_case(dims, M, n=600, nq=7)
    lists, codes = pqo.assign(oracle, 0, X, C), pqo.encode(oracle, cb, X)
    n = X.shape[0]
    full_l, full_d = pqo.brute(oracle, cb, Q, codes, n)  # the whole ranking
    lab, dist, scanned = pqo.search(oracle, cb, 0, Q, C, lists, codes, 10, 3)
    differ = 0
    for j in range(Q.shape[0]):
        pr = io.probes(oracle, 0, 0, Q[j], C, 3)
        keep = np.isin(lists[full_l[j]], pr)
        assert scanned[j] == keep.sum() and 0 < scanned[j] < n
        want_l, want_d = full_l[j][keep][:10], full_d[j][keep][:10]
        pad = 10 - want_l.size
        assert np.array_equal(lab[j], np.concatenate((want_l, np.full(pad, -1, np.int64))))
        assert np.array_equal(dist[j], np.concatenate((want_d, np.full(pad, pqo.FLT_MAX, pqo.F))))
        differ += int((lab[j] != full_l[j][:10]).any())
    assert differ > 0  # a search that ignored nprobe would not pass the GPU parity grid


def test_ties_resolve_to_the_lower_row_and_ids_follow(oracle):
    X, Q, C, cb = pqo.parity_case(16, 4, n=200, nq=4)
    X3 = np.concatenate((X, X, X))
    lists, codes = pqo.assign(oracle, 0, X3, C), pqo.encode(oracle, cb, X3)
    assert np.array_equal(codes[:200], codes[200:400]) and np.array_equal(lists[:200], lists[400:])
    lab, dist, _ = pqo.search(oracle, cb, 0, Q, C, lists, codes, 10, 16)
    for j in range(Q.shape[0]):
        assert dist[j, 0] == dist[j, 1] == dist[j, 2]
        assert lab[j, 0] < 200 and lab[j, 1] == lab[j, 0] + 200 and lab[j, 2] == lab[j, 0] + 400  # a tie group comes in row order
        assert lab[j, 9] < 200  # k = 10 cuts the fourth group after its first (lowest) row
    ids = np.arange(600, dtype=np.int64)[::-1] * 3 + (1 << 41)
    lab_i, dist_i, _ = pqo.search(oracle, cb, 0, Q, C, lists, codes, 10, 16, ids=ids)
    assert np.array_equal(lab_i, ids[lab]) and np.array_equal(dist_i, dist)  # ordered by row, labelled by id


def test_edge_case_shape(oracle):
    """what the GPU list-edge case relies on: the forced counts, a probed list longer than the scan's grid of tiles covers in one
    step, and a query whose positions cross several list boundaries inside one wave"""
    X, Q, C, owner, cb = pqo.edge_case()
    assert np.array_equal(pqo.assign(oracle, 0, X, C), owner)
    assert np.bincount(owner, minlength=len(pqo.EDGE_COUNTS)).tolist() == list(pqo.EDGE_COUNTS)
    nlist = C.shape[0]
    assert Q.shape[0] == 6 * nlist
    assert [int(io.probes(oracle, 0, 0, Q[i], C, 1)[0]) for i in range(Q.shape[0])] == list(range(nlist)) * 6
    long_list = pqo.EDGE_COUNTS[pqo.EDGE_LONG]
    groups = pqo.scan_groups(Q.shape[0], long_list)  # nprobe = 1: pmax is the longest list
    assert groups * pqo.TILE < long_list  # the stride loop takes a second step
    most = 0
    for j in range(Q.shape[0]):  # every list probed: the boundaries between the slots, in probe order
        seg = np.cumsum([pqo.EDGE_COUNTS[int(l)] for l in io.probes(oracle, 0, 0, Q[j], C, nlist)])[:-1]
        most = max(most, int(np.bincount(seg // 64).max()))
    assert most >= 3

