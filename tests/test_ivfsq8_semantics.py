"""tests/ivfsq8_oracle.py against the brute-force integer ranking, and the conditions tests/test_gpu_ivfsq8.py relies on in its
inputs, asserted here on the CPU instead of assumed there."""
import numpy as np
import pytest

from tests import ivf_oracle as io
from tests import ivfsq8_oracle as sqo
from tests import sq8_oracle as so


def test_the_rounding_case_is_the_trap(oracle):
    """two S above 2^24 that round to one float: the integers' order is not the floats'"""
    X, Q, C, mn, mx = sqo.rounding_case()
    assert X.shape == (4, 264) and (so.params(mn, mx)[0] == 1.0).all()
    codes = sqo.encode(X, mn, mx)
    assert np.array_equal(codes, X.astype(np.uint8))  # integer-valued rows encode to themselves
    qc = sqo.encode(Q, mn, mx)
    assert not qc.any()
    S = so.dist_s(qc[0], codes)
    assert S.tolist() == [16777217, 16777216, 16777217, 16777216] == list(sqo.ROUNDING_S)
    assert (S.astype(np.float32) == np.float32(16777216.0)).all()  # all four round to one float
    lists = sqo.assign(oracle, 0, X, C)
    lab, dist, scanned = sqo.search(oracle, 0, Q, C, lists, codes, mn, mx, 4, 2)
    assert lab[0].tolist() == [1, 3, 0, 2] and (dist[0] == np.float32(16777216.0)).all() and scanned[0] == 4
    by_float = np.lexsort((np.arange(4), S.astype(np.float32)))  # what pack_entry(float(S), row) would sort by
    assert by_float.tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("dims", [16, 20])
@pytest.mark.parametrize("order", [0, 1])
def test_every_list_probed_is_the_flat_sq8_search(oracle, dims, order):
    X, Q, C, mn, mx = sqo.parity_case(dims, n=600, nq=5)
    lists, codes = sqo.assign(oracle, order, X, C), sqo.encode(X, mn, mx)
    bl, bd = sqo.brute(Q, codes, mn, mx, 10)
    fl, fd = so.search(so.encode(Q, mn, mx), codes, 10)
    assert np.array_equal(bl, fl) and np.array_equal(bd, fd)
    for nprobe in (C.shape[0], C.shape[0] + 5):
        lab, dist, scanned = sqo.search(oracle, order, Q, C, lists, codes, mn, mx, 10, nprobe)
        assert np.array_equal(lab, bl) and np.array_equal(dist, bd)
        assert (scanned == X.shape[0]).all()
    mask = (np.random.default_rng(3).random(X.shape[0]) < 0.1).astype(np.uint8)
    vis = np.flatnonzero(mask)
    lab, dist, scanned = sqo.search(oracle, order, Q, C, lists, codes, mn, mx, 10, C.shape[0], mask=mask)
    ml, md = so.search(so.encode(Q, mn, mx), codes[vis], 10)
    assert np.array_equal(lab, np.where(ml >= 0, vis[np.clip(ml, 0, None)], -1)) and np.array_equal(dist, md)
    assert (scanned == vis.size).all()


def test_result_is_the_brute_ranking_restricted_to_the_probed_rows(oracle):
    X, Q, C, mn, mx = sqo.parity_case(16, n=600, nq=7)
    lists, codes = sqo.assign(oracle, 0, X, C), sqo.encode(X, mn, mx)
    n = X.shape[0]
    full_l, full_d = sqo.brute(Q, codes, mn, mx, n)  # the whole ranking
    lab, dist, scanned = sqo.search(oracle, 0, Q, C, lists, codes, mn, mx, 10, 3)
    differ = 0
    for j in range(Q.shape[0]):
        keep = np.isin(lists[full_l[j]], io.probes(oracle, 0, 0, Q[j], C, 3))
        assert scanned[j] == keep.sum() and 0 < scanned[j] < n
        want_l, want_d = full_l[j][keep][:10], full_d[j][keep][:10]
        pad = 10 - want_l.size
        assert np.array_equal(lab[j], np.concatenate((want_l, np.full(pad, -1, np.int64))))
        assert np.array_equal(dist[j], np.concatenate((want_d, np.full(pad, sqo.FLT_MAX, sqo.F))))
        differ += int((lab[j] != full_l[j][:10]).any())
    assert differ > 0  # a search that ignored nprobe would not pass the GPU parity grid
    ids = np.arange(n, dtype=np.int64)[::-1] * 3 + (1 << 41)
    lab_i, dist_i, _ = sqo.search(oracle, 0, Q, C, lists, codes, mn, mx, 10, 3, ids=ids)
    assert np.array_equal(lab_i, np.where(lab >= 0, ids[np.clip(lab, 0, None)], -1)) and np.array_equal(dist_i, dist)


def test_parity_shapes_cover_the_scan_s_forms():
    """one piece; a padded stride; a partial chunk alone; one full chunk of a row's pieces plus a partial one; the workload's
    row, whole chunks only"""
    assert set((16, 20, 80, 768)) <= set(sqo.PARITY_DIMS)
    stride = {d: (d + 15) // 16 * 16 for d in sqo.PARITY_DIMS}
    pieces = {d: stride[d] // 16 for d in sqo.PARITY_DIMS}
    assert pieces[16] == 1 and stride[20] == 32 and 1 < pieces[80] < sqo.CHUNK
    assert pieces[144] // sqo.CHUNK == 1 and pieces[144] % sqo.CHUNK == 1
    assert pieces[768] % sqo.CHUNK == 0 and pieces[768] // sqo.CHUNK == 6


def test_edge_case_shape(oracle):
    """what the GPU list-edge case relies on: the forced counts, a probed list longer than the scan's grid of tiles covers in one
    step at the case's query count, and a query whose positions cross several list boundaries inside one wave"""
    X, Q, C, owner, mn, mx = sqo.edge_case()
    T = sqo.TILE
    assert sqo.EDGE_COUNTS[:5] == (0, 1, T - 1, T, T + 1)
    assert np.array_equal(sqo.assign(oracle, 0, X, C), owner)
    assert np.bincount(owner, minlength=len(sqo.EDGE_COUNTS)).tolist() == list(sqo.EDGE_COUNTS)
    nlist = C.shape[0]
    assert Q.shape[0] == sqo.EDGE_PER_LIST * nlist
    assert [int(io.probes(oracle, 0, 0, Q[i], C, 1)[0]) for i in range(Q.shape[0])] == list(range(nlist)) * sqo.EDGE_PER_LIST
    long_list = sqo.EDGE_COUNTS[sqo.EDGE_LONG]
    assert long_list == max(sqo.EDGE_COUNTS)
    gx = sqo.scan_tiles_x(Q.shape[0], long_list)  # nprobe = 1: a pair per query
    assert gx * T < long_list  # a workgroup takes a second tile
    assert sqo.scan_tiles_x(Q.shape[0] * nlist, long_list) * T < long_list  # and with every list probed
    most = 0
    for j in range(nlist):  # every list probed: the boundaries between the slots, in probe order
        seg = np.cumsum([sqo.EDGE_COUNTS[int(l)] for l in io.probes(oracle, 0, 0, Q[j], C, nlist)])[:-1]
        most = max(most, int(np.bincount(seg // 64).max()))
    assert most >= 3
    codes = sqo.encode(X, mn, mx)
    for l in (2, 3, 4, 5):  # the codes of a list differ: a scan that read one row for all would not pass
        assert np.unique(codes[owner == l], axis=0).shape[0] > 1


def test_skew_case_shape(oracle):
    X, Q, C, mn, mx = sqo.skew_case()
    sizes = np.bincount(sqo.assign(oracle, 0, X, C), minlength=C.shape[0])
    assert sizes[0] > sqo.LDS_KEYS and 2048 < sizes[2] <= sqo.LDS_KEYS and sizes[1] == sizes[3] == 0
    first = [int(io.probes(oracle, 0, 0, q, C, 1)[0]) for q in Q]
    assert first == [0, 0, 0, 2, 2]
