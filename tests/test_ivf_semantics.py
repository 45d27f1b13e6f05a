"""tests/ivf_oracle.py against the brute-force oracle, and the conditions tests/test_gpu_ivf.py relies on in its inputs, asserted
here on the CPU instead of assumed there."""
import numpy as np
import pytest

from tests import ivf_oracle as io


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("order", [0, 1])
def test_every_list_probed_is_brute_force(oracle, metric, order):
    X, Q, C = io.parity_case(n=600, nq=5)
    lists = io.assign(oracle, metric, order, X, C)
    bl, bd = io.brute(oracle, metric, order, Q, X, 10)
    for nprobe in (C.shape[0], C.shape[0] + 5):
        lab, dist, scanned = io.search(oracle, metric, order, Q, X, C, lists, 10, nprobe)
        assert np.array_equal(lab, bl) and np.array_equal(dist, bd)
        assert (scanned == X.shape[0]).all()


def test_ids_and_padding(oracle):
    X, Q, C, owner = io.edge_case((0, 1, 5))
    lists = io.assign(oracle, 0, 0, X, C)
    assert np.array_equal(lists, owner)  # (the noise is far below the centroids' spacing)
    ids = np.arange(X.shape[0], dtype=np.int64) * 7 + (1 << 41)
    lab, dist, scanned = io.search(oracle, 0, 0, Q, X, C, lists, 3, 1, ids=ids)
    assert scanned.tolist() == [0, 1, 5]
    assert (lab[0] == -1).all() and (dist[0] == io.FLT_MAX).all()
    assert lab[1, 0] == ids[np.flatnonzero(owner == 1)[0]] and (lab[1, 1:] == -1).all()
    assert (lab[2] >= 1 << 41).all() and (np.diff(dist[2]) >= 0).all()


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_parity_grid_distinguishes_nprobe(oracle, metric):
    """at nprobe = 3 most queries' lists differ from brute force (29, 33 and 33 of 33 for L2, cosine and dot): a search that
    ignored nprobe would fail the GPU parity grid"""
    X, Q, C = io.parity_case()
    lists = io.assign(oracle, metric, 0, X, C)
    lab, dist, scanned = io.search(oracle, metric, 0, Q, X, C, lists, 10, 3)
    bl, _ = io.brute(oracle, metric, 0, Q, X, 10)
    differ = int((lab != bl).any(axis=1).sum())
    assert differ == (29, 33, 33)[metric]  # of 33, for this generator and seed
    assert (scanned < X.shape[0]).all() and (scanned > 0).all()


def test_skew_case_shape(oracle):
    """list 0 holds more rows than any LDS selection could (32,768 keys and beyond), list 2 fewer than the 16,384 the selection
    copies to LDS, two lists are empty; the queries' first probes are lists 0, 0, 0, 2, 2"""
    X, Q, C = io.skew_case()
    lists = io.assign(oracle, 0, 0, X, C)
    sizes = np.bincount(lists, minlength=4)
    assert sizes[0] > 32768 and sizes[1] == 0 and sizes[3] == 0
    assert 2048 * 2 < sizes[2] <= 16384
    assert [int(io.probes(oracle, 0, 0, q, C, 1)[0]) for q in Q] == [0, 0, 0, 2, 2]


def test_k_edge_case_shape(oracle):
    counts = (2047, 2048, 2049)
    X, Q, C, owner = io.edge_case(counts)
    assert np.array_equal(io.assign(oracle, 0, 0, X, C), owner)
    assert [int(io.probes(oracle, 0, 0, Q[i], C, 1)[0]) for i in range(3)] == [0, 1, 2]
