"""tests/ivfbq_oracle.py against the brute-force Hamming ranking, and the conditions tests/test_gpu_ivfbq.py relies on in its
inputs, asserted here on the CPU instead of assumed there."""
import numpy as np
import pytest

from tests import bq_oracle as bo
from tests import ivf_oracle as io
from tests import ivfbq_oracle as bqo


@pytest.mark.parametrize("dims", [16, 100])
@pytest.mark.parametrize("order", [0, 1])
def test_every_list_probed_is_the_flat_bq_search(oracle, dims, order):
    X, Q, C = bqo.parity_case(dims, n=600, nq=5)
    lists, codes = bqo.assign(oracle, order, X, C), bqo.encode(X)
    bl, bd = bqo.brute(Q, codes, 10)
    fl, fd = bo.search(bo.encode(Q), codes, 10)
    assert np.array_equal(bl, fl) and np.array_equal(bd, fd)
    for nprobe in (C.shape[0], C.shape[0] + 5):
        lab, dist, scanned = bqo.search(oracle, order, Q, C, lists, codes, 10, nprobe)
        assert np.array_equal(lab, bl) and np.array_equal(dist, bd)
        assert (scanned == X.shape[0]).all()
    mask = (np.random.default_rng(3).random(X.shape[0]) < 0.1).astype(np.uint8)
    vis = np.flatnonzero(mask)
    lab, dist, scanned = bqo.search(oracle, order, Q, C, lists, codes, 10, C.shape[0], mask=mask)
    ml, md = bo.search(bo.encode(Q), codes[vis], 10)
    assert np.array_equal(lab, np.where(ml >= 0, vis[np.clip(ml, 0, None)], -1)) and np.array_equal(dist, md)
    assert (scanned == vis.size).all()


def test_result_is_the_brute_ranking_restricted_to_the_probed_rows(oracle):
    X, Q, C = bqo.parity_case(100, n=600, nq=7)
    lists, codes = bqo.assign(oracle, 0, X, C), bqo.encode(X)
    n = X.shape[0]
    full_l, full_d = bqo.brute(Q, codes, n)  # the whole ranking
    lab, dist, scanned = bqo.search(oracle, 0, Q, C, lists, codes, 10, 3)
    differ = 0
    for j in range(Q.shape[0]):
        keep = np.isin(lists[full_l[j]], io.probes(oracle, 0, 0, Q[j], C, 3))
        assert scanned[j] == keep.sum() and 0 < scanned[j] < n
        want_l, want_d = full_l[j][keep][:10], full_d[j][keep][:10]
        pad = 10 - want_l.size
        assert np.array_equal(lab[j], np.concatenate((want_l, np.full(pad, -1, np.int64))))
        assert np.array_equal(dist[j], np.concatenate((want_d, np.full(pad, bqo.FLT_MAX, bqo.F))))
        differ += int((lab[j] != full_l[j][:10]).any())
    assert differ > 0  # a search that ignored nprobe would not pass the GPU parity grid
    ids = np.arange(n, dtype=np.int64)[::-1] * 3 + (1 << 41)
    lab_i, dist_i, _ = bqo.search(oracle, 0, Q, C, lists, codes, 10, 3, ids=ids)
    assert np.array_equal(lab_i, np.where(lab >= 0, ids[np.clip(lab, 0, None)], -1)) and np.array_equal(dist_i, dist)


def test_parity_shapes_cover_the_scan_s_forms():
    """W = 1 and W = 2 with pad bits in a chunk of 4; the workload's 12 words as one chunk; the 16-word boundary of the single
    chunk; 17 words as two chunks of 8 plus a partial one"""
    assert bqo.PARITY_DIMS == (16, 100, 768, 1024, 1088)
    W = {d: bo.words(d) for d in bqo.PARITY_DIMS}
    assert W[16] == 1 and 16 % 64 != 0 and bqo.chunk_words(1) == 4
    assert W[100] == 2 and 100 % 64 != 0 and bqo.chunk_words(2) == 4
    assert W[768] == 12 and bqo.chunk_words(12) == 12 and bqo.chunks(12) == 1
    assert W[1024] == 16 and bqo.chunk_words(16) == 16 and bqo.chunks(16) == 1
    assert W[1088] == 17 and bqo.chunk_words(17) == 8 and bqo.chunks(17) == 3 and 17 % 8 == 1
    assert {bqo.chunk_words(w) for w in range(1, 129)} == {4, 8, 12, 16}
    # pad bits stay zero in the codes and a NaN component gives bit 0
    v = np.full((1, 100), 1.0, np.float32)
    v[0, 5] = np.nan
    c = bo.encode(v)
    assert c.shape == (1, 2) and int(c[0, 1]) == (1 << 36) - 1 and int(c[0, 0]) == (1 << 64) - 1 - (1 << 5)


def test_ties_span_lists(oracle):
    """at dims 16 a distance takes 17 values: every query's top 10 of the tripled rows holds tie groups whose rows lie in
    different lists, so that the scan, which sees them list by list, does not meet them in row order"""
    X3, Q, C = bqo.tie_case()
    n = X3.shape[0] // 3
    assert np.array_equal(X3[:n], X3[n:2 * n]) and np.array_equal(X3[:n], X3[2 * n:])
    lists, codes = bqo.assign(oracle, 0, X3[:n], C), bqo.encode(X3[:n])
    lists3, codes3 = np.tile(lists, 3), np.tile(codes, (3, 1))
    lab, dist, _ = bqo.search(oracle, 0, Q, C, lists3, codes3, 10, 16)
    assert (lab >= 0).all()
    qc = bo.encode(Q)
    for j in range(Q.shape[0]):
        assert np.unique(dist[j]).size < 10  # ties inside the top 10
        h = bo.hamming(qc[j], codes3)
        spans = False
        for d in np.unique(dist[j]):
            got = lab[j][dist[j] == d]
            group = np.flatnonzero(h == int(d))  # every row at this distance: the result holds the first of them, by row
            assert np.array_equal(got, group[:got.size])
            spans = spans or np.unique(lists3[group]).size > 1
        assert spans, j
    # and in probe order the lists are not ascending for every query: list-by-list is not row order
    assert any((np.diff(io.probes(oracle, 0, 0, q, C, 16)) < 0).any() for q in Q)


def test_edge_case_shape(oracle):
    """what the GPU list-edge case relies on: the forced counts, a probed list longer than the scan's grid of tiles covers in one
    step at the case's query count, and a query whose positions cross several list boundaries inside one wave"""
    X, Q, C, owner = bqo.edge_case()
    T = bqo.TILE
    assert T == 256 and bqo.GRID == 4096 and bqo.LDS_KEYS == 16384
    assert bqo.EDGE_COUNTS == (0, 1, T - 1, T, T + 1, 17 * T + 77, 3, 5, 2, 0, 7)
    assert np.array_equal(bqo.assign(oracle, 0, X, C), owner)
    assert np.bincount(owner, minlength=len(bqo.EDGE_COUNTS)).tolist() == list(bqo.EDGE_COUNTS)
    nlist = C.shape[0]
    assert Q.shape[0] == bqo.EDGE_PER_LIST * nlist
    assert [int(io.probes(oracle, 0, 0, Q[i], C, 1)[0]) for i in range(Q.shape[0])] == list(range(nlist)) * bqo.EDGE_PER_LIST
    long_list = bqo.EDGE_COUNTS[bqo.EDGE_LONG]
    assert long_list == max(bqo.EDGE_COUNTS) and -(-long_list // T) == 18
    gx = bqo.scan_tiles_x(Q.shape[0], long_list)  # nprobe = 1: a pair per query
    assert gx == 16 and gx * T < long_list  # a workgroup takes a second tile
    assert bqo.scan_tiles_x(Q.shape[0] * nlist, long_list) * T < long_list  # and with every list probed
    most = 0
    for j in range(nlist):  # every list probed: the boundaries between the slots, in probe order
        seg = np.cumsum([bqo.EDGE_COUNTS[int(l)] for l in io.probes(oracle, 0, 0, Q[j], C, nlist)])[:-1]
        most = max(most, int(np.bincount(seg // 64).max()))
    assert most >= 3
    codes = bqo.encode(X)
    for l in (2, 3, 4, 5):  # the codes of a list differ: a scan that read one row for all would not pass
        assert np.unique(codes[owner == l], axis=0).shape[0] > 1


def test_skew_case_shape(oracle):
    X, Q, C = bqo.skew_case()
    sizes = np.bincount(bqo.assign(oracle, 0, X, C), minlength=C.shape[0])
    assert sizes[0] > bqo.LDS_KEYS and 2048 < sizes[2] <= bqo.LDS_KEYS and sizes[1] == sizes[3] == 0
    first = [int(io.probes(oracle, 0, 0, q, C, 1)[0]) for q in Q]
    assert first == [0, 0, 0, 2, 2]
