"""tests/ivfpq_residual_oracle.py on the CPU: what tests/test_gpu_ivfpq_residual.py relies on in the shared inputs, the one case
in which a residual handle equals the plain one, and the pure host rules of the residual search (the scan's grid, the table
budget), asserted here instead of assumed there."""
import numpy as np
import pytest

from tests import ivf_oracle as io
from tests import ivfpq_oracle as pqo
from tests import ivfpq_residual_oracle as ro


def test_edge_case_takes_a_second_stride_step(oracle):
    X, Q, C, owner, cb = pqo.edge_case()
    assert np.array_equal(pqo.assign(oracle, 0, X, C), owner)
    assert np.bincount(owner, minlength=len(pqo.EDGE_COUNTS)).tolist() == list(pqo.EDGE_COUNTS)
    long_list = pqo.EDGE_COUNTS[pqo.EDGE_LONG]
    assert long_list == max(pqo.EDGE_COUNTS) and Q.shape[0] == 66
    groups = ro.rscan_groups(Q.shape[0] * 1, long_list)  # nprobe = 1: a pair a query
    assert groups == 8 and groups * ro.TILE < long_list  # the long list's workgroups take a second step
    nlist = C.shape[0]
    g = ro.rscan_groups(Q.shape[0] * nlist, long_list)  # every list probed
    tiles = [-(-c // ro.TILE) for c in pqo.EDGE_COUNTS if c > 0]
    assert g >= 1 and g <= min(tiles)  # never more workgroups than a (non-empty) list has tiles


@pytest.mark.parametrize("pairs,maxlen,want", [
    (1, 0, 1), (1, 1, 1), (1, 1024, 1), (1, 1025, 2), (1, 10 ** 7, 512), (8, 313888, 64), (64, 313888, 8), (512, 313888, 1),
    (513, 313888, 1), (2048, 313888, 1), (3, 2048, 2), (66, 8269, 8), (171, 8269, 3),
])
def test_rscan_groups(pairs, maxlen, want):
    """G = clamp(ceil(IPQ_GRID / pairs), 1, ceil(maxlen / IPQ_TILE))"""
    assert ro.rscan_groups(pairs, maxlen) == want


def test_the_gpu_cases_take_both_forms_of_the_scan():
    """the strided grid while the longest list is at most two stride steps, the work list beyond; on the edge case the GPU test
    runs the stride loop's second step (nprobe = 1) and work lists of 2 and 3 tiles an item, the long list's 9 tiles cut in runs"""
    counts = sorted(pqo.EDGE_COUNTS, reverse=True)
    nq, long_list = 66, counts[0]
    assert ro.rscan_plan(nq * 1, nq, long_list, long_list) == ("strided", 8)
    assert ro.rscan_plan(nq * 2, nq, sum(counts[:2]), long_list) == ("items", 2, 132 + 366)
    assert ro.rscan_plan(nq * 5, nq, sum(counts[:5]), long_list) == ("items", 3, 330 + 354)
    assert ro.rscan_plan(nq * 11, nq, sum(counts), long_list) == ("items", 3, 726 + 487)
    # the plan's bound of the items holds for any split of nq * pmax positions over the pairs
    rng = np.random.default_rng(0)
    for _ in range(200):
        nq, np_ = int(rng.integers(1, 70)), int(rng.integers(1, 40))
        lens = rng.integers(0, 9000, (nq, np_)) * (rng.random((nq, np_)) < 0.7)
        pmax, maxlen = int(lens.sum(axis=1).max()), int(lens.max())
        plan = ro.rscan_plan(nq * np_, nq, max(pmax, 1), maxlen)
        if plan[0] == "items":
            items = -(-(-(-lens // ro.TILE)) // plan[1])
            assert 1 <= plan[1] <= ro.RUN_MAX and int(items.sum()) <= plan[2]
        else:
            assert -(-maxlen // ro.TILE) <= 2 * plan[1]
    # the bench shape (10M rows, longest list 313,888): one query keeps the strided grid at one probe and leaves it at eight
    assert ro.rscan_plan(1, 1, 313888, 313888) == ("strided", 307)
    assert ro.rscan_plan(8, 1, 1_300_000, 313888)[0] == "items"


@pytest.mark.parametrize("dims,M", pqo.PARITY_SHAPES)
def test_parity_centroids_have_zero_residuals(oracle, dims, M):
    X, Q, C, cb = pqo.parity_case(dims, M)
    lists = pqo.assign(oracle, 0, X, C)
    res = ro.residuals(X, C, lists)
    zero = np.flatnonzero((res == 0).all(axis=1))
    assert zero.size >= C.shape[0]  # the centroids are rows: each is its own list's centre
    assert set(lists[zero].tolist()) == set(range(C.shape[0]))
    assert np.array_equal(res[5], (X[5] - C[lists[5]]).astype(np.float32))


def test_zero_centroid_equals_the_plain_oracle(oracle):
    """centroids (0, +1e6, -1e6) in every coordinate: every row lands in list 0 and x - 0 = x, so codes, labels and distances
    are the plain handle's, bit for bit, whenever list 0 is probed first (every query is standard-normal too)"""
    X, Q, C, cb = ro.zero_centroid_case()
    lists = pqo.assign(oracle, 0, X, C)
    assert (lists == 0).all()
    codes = ro.encode(oracle, cb, X, C, lists)
    assert np.array_equal(codes, pqo.encode(oracle, cb, X))
    for nprobe in (1, 2, 3):
        rl, rd, rs = ro.search(oracle, cb, 0, Q, C, lists, codes, 10, nprobe)
        pl, pd, ps = pqo.search(oracle, cb, 0, Q, C, lists, codes, 10, nprobe)
        assert np.array_equal(rl, pl) and np.array_equal(rd, pd) and np.array_equal(rs, ps)
        assert (rs == X.shape[0]).all()


def test_residual_search_differs_from_the_plain_one_and_honours_masks_and_ids(oracle):
    X, Q, C, cb = pqo.parity_case(16, 4, n=600, nq=7)
    lists = pqo.assign(oracle, 0, X, C)
    codes = ro.encode(oracle, cb, X, C, lists)
    assert not np.array_equal(codes, pqo.encode(oracle, cb, X))
    rl, rd, rs = ro.search(oracle, cb, 0, Q, C, lists, codes, 10, 3)
    pl, pd, ps = pqo.search(oracle, cb, 0, Q, C, lists, codes, 10, 3)
    assert np.array_equal(rs, ps) and not np.array_equal(rd, pd)  # the same rows scanned, under other tables
    for j in range(Q.shape[0]):  # each distance is the per-list table's
        r = int(rl[j, 0])
        table = oracle.build_adc_table(cb, (Q[j] - C[lists[r]]).astype(np.float32))
        assert oracle.adc_batch(table, codes[r:r + 1])[0] == rd[j, 0]
        assert np.isin(lists[rl[j][rl[j] >= 0]], io.probes(oracle, 0, 0, Q[j], C, 3)).all()
    mask = (np.arange(600) % 3 != 0).astype(np.uint8)
    ml, md, ms = ro.search(oracle, cb, 0, Q, C, lists, codes, 10, 3, visible=mask)
    assert (mask[ml[ml >= 0]] != 0).all() and (ms < rs).all()
    ids = np.arange(600, dtype=np.int64)[::-1] * 3 + (1 << 41)
    il, idd, _ = ro.search(oracle, cb, 0, Q, C, lists, codes, 10, 3, ids=ids)
    assert np.array_equal(il, np.where(rl >= 0, ids[np.clip(rl, 0, None)], -1)) and np.array_equal(idd, rd)


def test_table_budget():
    """nb shrinks so that nb * np * M * 1024 <= 2^30; rounds of slots only when one query's tables do not fit"""
    for M in (1, 4, 16, 96, 159):
        for np_ in (1, 8, 130, 1024, 6594, 6595, 6600, 10922, 10923, 65536):
            nb, slots = ro.table_plan(np_, M)
            assert nb >= 1 and 1 <= slots <= np_
            assert nb * slots * M * 1024 <= ro.TABLE_SCRATCH
            if slots < np_:
                assert nb == 1 and np_ * M * 1024 > ro.TABLE_SCRATCH
                assert (slots + 1) * M * 1024 > ro.TABLE_SCRATCH  # as many slots a round as fit
            else:
                assert (nb + 1) * np_ * M * 1024 > ro.TABLE_SCRATCH  # as many queries a batch as fit
    assert ro.table_plan(1, 96) == (10922, 1)  # at M = 96 room for 10,922 tables
    assert ro.table_plan(16, 96) == (682, 16) and ro.batch_queries(700, 16, 96) == 682
    assert ro.table_plan(130, 159) == (50, 130) and ro.batch_queries(120, 130, 159) == 50
    assert ro.batch_queries(5000, 3, 4) == ro.QUERY_BATCH
    assert ro.slot_rounds(6594, 159) == 1 and ro.slot_rounds(6595, 159) == 2  # at M = 159 from 6,595 probes
    assert ro.table_plan(6600, 159) == (1, 6594) and ro.slot_rounds(6600, 159) == 2
