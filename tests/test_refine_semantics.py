"""lb_gpu_index_refine without a device: the three entry points are declared and exported, a null handle is refused before
anything is touched, the Python front end has its methods, and tests/refine_oracle.py (the restatement the GPU tests compare
against, tests/test_gpu_refine.py) gives what include/longbow_gpu.h states on cases written out by hand."""
import os

import numpy as np
import pytest

from tests import refine_oracle as fo

F = np.float32
INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lb_gpu_index_refine", "lb_gpu_index_refine_ctx", "lb_gpu_index_refine_device_ctx")


@pytest.fixture(scope="module")
def lib():
    from longbow_amd import _lib
    return _lib.load()


def test_the_entry_points_are_declared_and_exported(lib):
    with open(os.path.join(ROOT, "include", "longbow_gpu.h")) as f:
        header = f.read()
    assert "#define LB_REFINE_MAX_C 16384" in header
    for name in NAMES:
        assert f"int {name}(lb_gpu_index *h, int64_t nq, const float *" in header, name
        assert getattr(lib, name) is not None, name


def test_null_handle_is_refused_and_nothing_is_written(lib):
    nq, dim, c, k = 2, 4, 3, 2
    q = np.full((nq, dim), 7.0, F)
    rows = np.arange(nq * c, dtype=np.int64).reshape(nq, c)
    dist = np.full((nq, k), 9.0, F)
    lab = np.full((nq, k), 77, np.int64)
    a = (q.ctypes.data, c, rows.ctypes.data)
    for n in (nq, 0, -1):
        for kk in (k, 0, 2048, 2049):  # INVALID_ARG comes before UNSUPPORTED
            for order in (-1, 0, 1, 5):
                assert lib.lb_gpu_index_refine(None, n, *a, kk, order, dist.ctypes.data, lab.ctypes.data) == INVALID
                assert lib.lb_gpu_index_refine_ctx(None, n, *a, kk, order, dist.ctypes.data, lab.ctypes.data, None) == INVALID
                assert lib.lb_gpu_index_refine_device_ctx(None, n, *a, kk, order, dist.ctypes.data, lab.ctypes.data, None, None) == INVALID
    assert (q == 7.0).all() and (rows == np.arange(nq * c).reshape(nq, c)).all() and (dist == 9.0).all() and (lab == 77).all()


def test_python_front_end_has_the_methods():
    from longbow_amd import _ivfbase, bq, gpu, ivfpq, pq, sq8
    assert callable(gpu.Index.Refine) and callable(gpu.Index.refine_device)
    for cls in (bq.BQEncoder, sq8.SQ8Encoder, pq.PQEncoder, ivfpq.IVFPQ):
        assert callable(cls.search_refine), cls
    assert _ivfbase.IVFBase._has_ids is False


# ---- the oracle on hand-written cases: rows on a line, the query at the origin, so that an L2 distance is the row's coordinate --------
@pytest.fixture(scope="module")
def line():
    X = np.array([[0], [1], [2], [3], [4], [2]], F)  # rows 2 and 5 are the same vector
    return X, np.zeros((1, 1), F)


def test_oracle_duplicates_invalid_entries_and_order(oracle, line):
    X, Q = line
    assert fo.clean([3, 3, -1, 1, 6, 2 ** 40, 1, -(2 ** 62)], 6).tolist() == [1, 3]
    lab, dist = fo.refine(oracle, 0, Q, X, [[3, 3, -1, 1, 6, 2 ** 40, 1, -(2 ** 62)]], 2, 0)
    assert lab.tolist() == [[1, 3]] and dist.tolist() == [[1.0, 3.0]]
    again = fo.refine(oracle, 0, Q, X, [[1, 3]], 2, 0)
    assert np.array_equal(again[0], lab) and np.array_equal(again[1], dist)


def test_oracle_padding_and_k_beyond_the_set(oracle, line):
    X, Q = line
    lab, dist = fo.refine(oracle, 0, Q, X, [[4, 0, -1]], 4, 1)
    assert lab.tolist() == [[0, 4, -1, -1]]
    assert dist[0, :2].tolist() == [0.0, 4.0] and (dist[0, 2:] == fo.FLT_MAX).all()


def test_oracle_all_invalid_list_is_all_padding(oracle, line):
    X, Q = line
    lab, dist = fo.refine(oracle, 0, Q, X, [[-1, 6, 2 ** 40]], 3, 0)
    assert (lab == -1).all() and (dist == fo.FLT_MAX).all()
    lab, dist = fo.refine(oracle, 0, Q, np.zeros((0, 1), F), [[0, 1]], 2, 0)  # an empty index
    assert (lab == -1).all() and (dist == fo.FLT_MAX).all()


def test_oracle_ties_go_by_row_and_ids_map_last(oracle, line):
    X, Q = line
    lab, dist = fo.refine(oracle, 0, Q, X, [[5, 3, 2]], 3, 0)
    assert lab.tolist() == [[2, 5, 3]] and dist.tolist() == [[2.0, 2.0, 3.0]]
    ids = np.array([100, 90, 80, 70, 60, 50], np.int64)
    lab, _ = fo.refine(oracle, 0, Q, X, [[5, 3, 2]], 4, 0, ids=ids)
    assert lab.tolist() == [[80, 50, 70, -1]]  # ordered by row, reported as ids


def test_oracle_metrics(oracle):
    X = np.array([[1, 0], [0, 2], [-3, 0]], F)
    Q = np.array([[1, 0]], F)
    lab, dist = fo.refine(oracle, 2, Q, X, [[0, 1, 2]], 3, 0)  # dot, negated
    assert lab.tolist() == [[0, 1, 2]] and dist.tolist() == [[-1.0, 0.0, 3.0]]
    lab, dist = fo.refine(oracle, 1, Q, X, [[2, 1, 0]], 3, 0)  # cosine: 1 - cos
    assert lab.tolist() == [[0, 1, 2]] and dist.tolist() == [[0.0, 1.0, 2.0]]
