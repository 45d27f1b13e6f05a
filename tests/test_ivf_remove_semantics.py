"""The premise of tests/test_gpu_ivf_remove.py, pinned on the CPU with the oracle alone: the search of the live rows X[live] with
their lists lists[live] (and their ids, where given) IS the search of every row with the removed rows' lists set to -1, which is
what tests/ivf_remove_cases.py's search_live computes; without ids the fresh handle's labels are the survivors' new positions,
which np.flatnonzero(live) takes back.  Also the conditions the GPU file relies on in its inputs, asserted here instead of assumed
there."""
import numpy as np
import pytest

from tests import ivf_oracle as io
from tests import ivf_remove_cases as vc


def _back(labels, keep):
    """labels of the compacted corpus -> the old positions"""
    return np.where(labels >= 0, keep[np.clip(labels, 0, None)], -1)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_the_survivors_alone_answer_as_every_row_under_the_live_mask(oracle, metric):
    X, Q, C = io.parity_case()
    n = X.shape[0]
    lists = vc.parity_lists(oracle, metric)
    ids = vc.ids_for(n)
    for name in ("18pct", "60pct"):
        removed = vc.removed_rows(n, name)
        live = vc.live_mask(n, removed)
        keep = np.flatnonzero(live)
        Qr = vc.queries(X, Q, removed)[:9]
        for nprobe in vc.NPROBES:
            # the largest k once: a smaller k's answer is its prefix (canonical order), which the GPU file relies on too
            wl, wd, ws = vc.search_live(oracle, metric, 0, Qr, X, C, lists, live, vc.KS[-1], nprobe)
            fl, fd, fs = io.search(oracle, metric, 0, Qr, X[keep], C, lists[keep], vc.KS[-1], nprobe)
            assert np.array_equal(_back(fl, keep), wl) and np.array_equal(fd, wd) and np.array_equal(fs, ws), (name, nprobe)
            il, idist, _ = io.search(oracle, metric, 0, Qr, X[keep], C, lists[keep], vc.KS[-1], nprobe, ids=ids[keep])
            wil, wid, _ = vc.search_live(oracle, metric, 0, Qr, X, C, lists, live, vc.KS[-1], nprobe, ids=ids)
            assert np.array_equal(il, wil) and np.array_equal(idist, wid), (name, nprobe)
            for k in vc.KS[:-1]:
                kl, kd, _ = vc.search_live(oracle, metric, 0, Qr, X, C, lists, live, k, nprobe)
                assert np.array_equal(kl, wl[:, :k]) and np.array_equal(kd, wd[:, :k]), (name, nprobe, k)
            assert not np.isin(wl, removed).any()
        assert (ws == live.sum()).all()  # (nprobe = 16: every list probed, every live row scanned)


def test_the_live_mask_combines_with_a_filter(oracle):
    X, Q, C = io.parity_case()
    n = X.shape[0]
    lists = vc.parity_lists(oracle, 0)
    removed = vc.removed_rows(n, "18pct")
    live = vc.live_mask(n, removed)
    m = vc.filter_mask(n)
    m[removed[:20]] = 0x80
    both = vc.visible(live, m)
    keep = np.flatnonzero(live)
    assert 0 < both.sum() < live.sum() and (m[removed] != 0).any()
    for nprobe in vc.NPROBES:
        wl, wd, ws = vc.search_live(oracle, 0, 0, Q[:9], X, C, lists, live, 10, nprobe, mask=m)
        # the fresh handle of the survivors under the same filter restricted to them
        fl, fd, fs = io.search(oracle, 0, 0, Q[:9], X[keep], C, np.where(m[keep] != 0, lists[keep], -1), 10, nprobe)
        assert np.array_equal(_back(fl, keep), wl) and np.array_equal(fd, wd) and np.array_equal(fs, ws), nprobe
        assert both[wl[wl >= 0]].all()


def test_readback_sets(oracle):
    X, Q, C = io.parity_case()
    n = X.shape[0]
    lists = vc.parity_lists(oracle, 0)
    sets = vc.readback_sets(lists)
    assert tuple(sorted(sets)) == tuple(sorted(vc.READBACK_NAMES))
    assert sets["none"].size == 0 and sets["first"].tolist() == [0] and sets["last"].tolist() == [n - 1]
    assert sets["all"].size == n and sets["all but one"].size == n - 1 and sets["every other"].size == n // 2
    one = sets["one list"]
    assert 0 < one.size < n and np.unique(lists[one]).size == 1 and not (lists[np.setdiff1d(np.arange(n), one)] == lists[one[0]]).any()
    # query 0 of the GPU test is a removed row's own vector: without the removal that row is its nearest neighbour
    removed = sets["every other"]
    Qr = vc.queries(X, Q, removed)
    lab, dist, _ = io.search(oracle, 0, 0, Qr[:1], X, C, lists, 1, 16)
    assert lab[0, 0] == removed[len(removed) // 2] and dist[0, 0] == 0
    # n live rows or fewer than 2048: the k = 2048 search returns every live row
    assert n - sets["every other"].size <= 2048 < n


def test_list_edges_inputs(oracle):
    """list i is left exactly EDGE_KEEP[i] live rows, one list is emptied, and query i probes list i first; as int8 rows too"""
    for X, Q, C, owner in (io.edge_case(vc.EDGE_COUNTS), vc.edge_case_i8()):
        W, WQ = X.astype(vc.F), Q.astype(vc.F)
        assert np.array_equal(io.assign(oracle, 0, 0, W, C), owner)
        assert [int(io.probes(oracle, 0, 0, WQ[i], C, 1)[0]) for i in range(len(vc.EDGE_COUNTS))] == list(range(len(vc.EDGE_COUNTS)))
        for rng in (None, np.random.default_rng(6)):
            live = vc.live_mask(owner.size, vc.edge_removed(owner, rng))
            assert np.bincount(owner[live != 0], minlength=len(vc.EDGE_KEEP)).tolist() == list(vc.EDGE_KEEP)
        assert 0 in vc.EDGE_KEEP and {127, 128, 129} <= set(vc.EDGE_KEEP)
    X8 = vc.edge_case_i8()[0]
    assert np.unique(X8[owner == 5], axis=0).shape[0] > 100  # the int8 rows of a list differ


def test_selection_boundary_inputs(oracle):
    """the steps leave list 0 exactly LDS_KEYS + 1, LDS_KEYS and LDS_KEYS - 1 live rows, and the eight queries probe lists 0 and 2"""
    X, Q, C = io.skew_case()
    lists = io.assign(oracle, 0, 0, X, C)
    Q8 = vc.skew_queries(Q)
    assert Q8.shape[0] == 8
    first = [int(io.probes(oracle, 0, 0, q, C, 1)[0]) for q in Q8]
    assert first.count(0) == 6 and first.count(2) == 2
    live = np.ones(X.shape[0], np.uint8)
    assert np.count_nonzero(lists == 0) > vc.SKEW_KEEP[0] + 1000 and np.count_nonzero(lists == 2) <= vc.LDS_KEYS
    for keep0, rows in vc.skew_steps(lists):
        assert (live[rows] == 1).all() and (lists[rows] == 0).all()
        live[rows] = 0
        assert np.count_nonzero((lists == 0) & (live != 0)) == keep0
    assert vc.SKEW_KEEP == (vc.LDS_KEYS + 1, vc.LDS_KEYS, vc.LDS_KEYS - 1)
