"""The premise of tests/test_gpu_ivf_code_remove.py and tests/test_gpu_code_lifecycle.py, pinned on the CPU with the oracles alone,
for the IVF-PQ handle plain and residual and the IVF-SQ8 handle: each handle's oracle over ALL rows with
mask = live & filter IS that oracle over the survivors alone (their codes, their lists, the filter restricted to them) with ids
equal to the old labels; without ids the survivors' labels map back through old_rows.  That is the header's "a fresh handle with
the same centroids, codebooks or bounds that holds only the survivors' codes in their order".  Also the conditions the GPU file
relies on in its inputs (tests/ivf_code_remove_cases.py), asserted here instead of assumed there: this file pins the shapes."""
import numpy as np
import pytest

from tests import ivf_code_remove_cases as cc
from tests import ivf_oracle as io

NQ = 9  # the first queries of a case: query 0 is a removed row's own vector


@pytest.mark.parametrize("kind,shape", cc.SHAPES, ids=cc.SHAPE_IDS)
def test_the_survivors_alone_answer_as_every_row_under_the_live_mask(oracle, kind, shape):
    c = cc.parity(oracle, kind, shape)
    assert (c.n, c.nlist, c.Q.shape[0]) == (3000, 16, 33)
    ids = cc.ids_for(c.n)
    names = ("18pct", "60pct") if shape == cc.FIRST_SHAPE[kind] else ("18pct",)
    for name in names:
        removed = cc.removed_rows(c.n, name)
        live = cc.live_mask(c.n, removed)
        keep = np.flatnonzero(live)
        Q = cc.queries(c, removed)[:NQ]
        for nprobe in cc.NPROBES:
            # the largest k once: a smaller k's answer is its prefix (canonical order), which the GPU file relies on too
            wl, wd, ws = c.search(oracle, Q, live, cc.KS[-1], nprobe)
            fl, fd, fs = c.search(oracle, Q, np.ones(keep.size, np.uint8), cc.KS[-1], nprobe, rows=keep)
            assert np.array_equal(cc.back(fl, keep), wl) and np.array_equal(fd, wd) and np.array_equal(fs, ws), (name, nprobe)
            il, idist, _ = c.search(oracle, Q, np.ones(keep.size, np.uint8), cc.KS[-1], nprobe, ids=ids[keep], rows=keep)
            wil, wid, _ = c.search(oracle, Q, live, cc.KS[-1], nprobe, ids=ids)
            assert np.array_equal(il, wil) and np.array_equal(idist, wid), (name, nprobe)
            assert np.array_equal(wil, np.where(wl >= 0, ids[np.clip(wl, 0, None)], -1))
            for k in cc.KS[:-1]:
                kl, kd, _ = c.search(oracle, Q, live, k, nprobe)
                assert np.array_equal(kl, wl[:, :k]) and np.array_equal(kd, wd[:, :k]), (name, nprobe, k)
            assert not np.isin(wl, removed).any()
        assert (ws == live.sum()).all()  # (nprobe = 16: every list probed, every live row scanned)


@pytest.mark.parametrize("kind", list(cc.KINDS))
def test_the_live_mask_combines_with_a_filter(oracle, kind):
    c = cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])
    removed = cc.removed_rows(c.n, "18pct")
    live = cc.live_mask(c.n, removed)
    m = cc.filter_mask(c.n).copy()
    m[removed[:20]] = 0x80
    both = cc.visible(live, m)
    keep = np.flatnonzero(live)
    assert 0 < both.sum() < live.sum() and (m[removed] != 0).any()
    for nprobe in cc.NPROBES:
        wl, wd, ws = c.search(oracle, c.Q[:NQ], both, 10, nprobe)
        fl, fd, fs = c.search(oracle, c.Q[:NQ], m[keep], 10, nprobe, rows=keep)  # the survivors under the filter restricted to them
        assert np.array_equal(cc.back(fl, keep), wl) and np.array_equal(fd, wd) and np.array_equal(fs, ws), nprobe
        assert both[wl[wl >= 0]].all()


@pytest.mark.parametrize("kind", list(cc.KINDS))
def test_residual_codes_move_with_their_lists(oracle, kind):
    """what lets compaction keep the codes: the code of a survivor, encoded afresh from its vector among the survivors alone, is the
    code it had, because its list is a function of the row and the centroids alone (for a residual code: so is its residual)"""
    c = cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])
    keep = np.flatnonzero(cc.live_mask(c.n, cc.removed_rows(c.n, "60pct")))
    lists = c.k.assign(oracle, c.X[keep], c.C)
    assert np.array_equal(lists, c.lists[keep])
    assert np.array_equal(c.k.encode(oracle, c.X[keep], c.C, lists, c.par), c.codes[keep])
    if kind == "rpq":  # and the residual codes do depend on the list: they are not the plain codes
        assert not np.array_equal(c.codes, cc.parity(oracle, "pq", cc.FIRST_SHAPE["pq"]).codes)


@pytest.mark.parametrize("kind,shape", cc.SHAPES, ids=cc.SHAPE_IDS)
def test_readback_inputs(oracle, kind, shape):
    c = cc.parity(oracle, kind, shape)
    sets = cc.readback_sets(c.lists)
    assert tuple(sorted(sets)) == tuple(sorted(cc.READBACK_NAMES))
    one = sets["one list"]
    assert 0 < one.size < c.n and np.unique(c.lists[one]).size == 1
    assert c.n - sets["every other"].size <= cc.K_ALL < c.n  # k = 2048 returns every live row of "every other"
    # query 0 is a removed row's own vector: without the removal that row is a nearest neighbour at the handle's least distance
    removed = sets["every other"]
    Q = cc.queries(c, removed)
    lab, dist, _ = c.search(oracle, Q[:1], np.ones(c.n, np.uint8), cc.K_ALL, c.nlist)
    row = removed[len(removed) // 2]
    at = np.flatnonzero(lab[0] == row)
    assert at.size == 1 and dist[0, at[0]] == dist[0, 0]
    if kind == "sq8":
        assert dist[0, 0] == 0  # (its own code; a PQ code of a row is not the row)


@pytest.mark.parametrize("kind", list(cc.KINDS))
def test_list_edges_inputs(oracle, kind):
    """the keeps leave list i exactly keep[i] live rows: 0, 1, TILE - 1, TILE, TILE + 1 and several tiles plus a remainder"""
    c = cc.edge(oracle, kind)
    T = c.k.tile
    assert T == {"pq": 1024, "rpq": 1024, "sq8": 128}[kind]
    sizes = np.bincount(c.lists, minlength=c.nlist)
    assert sizes[:5].tolist() == [0, 1, T - 1, T, T + 1] and sizes[5] > 3 * T and sizes[5] % T
    assert np.array_equal(c.k.assign(oracle, c.X, c.C), c.lists)
    first = [int(io.probes(oracle, 0, 0, c.Q[i], c.C, 1)[0]) for i in range(c.Q.shape[0])]
    assert first == [i % c.nlist for i in range(c.Q.shape[0])]
    keeps = cc.edge_keeps(kind)
    seen = set()
    for name, keep in keeps.items():
        for rng in (None, np.random.default_rng(6)):
            removed = cc.edge_removed(c.lists, keep, rng)
            live = cc.live_mask(c.n, removed)
            assert np.bincount(c.lists[live != 0], minlength=c.nlist).tolist() == list(keep)
            assert removed.size > 0
        seen |= set(keep)
        assert any(k == 0 and s > 0 for k, s in zip(keep, sizes)), "a list emptied by the removal"
    assert {0, 1, T - 1, T, T + 1} <= seen
    assert any(k > 3 * T and k % T for k in keeps["B"])
    assert np.unique(c.codes[c.lists == 5], axis=0).shape[0] > 100


@pytest.mark.parametrize("kind", list(cc.KINDS))
def test_selection_boundary_inputs(oracle, kind):
    """the steps leave list 0 exactly LDS_KEYS + 1, LDS_KEYS and LDS_KEYS - 1 live rows; six of the eight queries probe it"""
    X, Q5, C, _ = cc.KINDS[kind].skew_case()
    lists = io.assign(oracle, 0, 0, X, C)
    Q8 = cc.vc.skew_queries(Q5)
    first = [int(io.probes(oracle, 0, 0, q, C, 1)[0]) for q in Q8]
    assert first.count(0) == 6 and first.count(2) == 2
    live = np.ones(X.shape[0], np.uint8)
    assert np.count_nonzero(lists == 0) > cc.SKEW_KEEP[0] + 1000 and np.count_nonzero(lists == 2) <= cc.LDS_KEYS
    for keep0, rows in cc.skew_steps(lists):
        assert (live[rows] == 1).all() and (lists[rows] == 0).all()
        live[rows] = 0
        assert np.count_nonzero((lists == 0) & (live != 0)) == keep0
    assert cc.SKEW_KEEP == (cc.LDS_KEYS + 1, cc.LDS_KEYS, cc.LDS_KEYS - 1)


def test_overlap_sets_and_ids():
    n = 3000
    sets = cc.overlap_sets(n)
    assert sets["row 0"].tolist() == [0] and sets["first half"].size == n // 2 and sets["every other"].size == n // 2
    assert any((n - s.size) % cc.ROUND_ROWS for s in sets.values())  # a partial last round of 7 rows
    ids = cc.ids_for(n)
    assert ids.min() < 0 and ids.max() > 2 ** 32 and np.unique(ids).size == n
