"""The premise of the removal tests, on the oracle alone: a search over the live rows only, X[live] with ids = labels[live], is the
search over every row under mask = live with ids = labels.  The GPU tests compare the index against the second form and against
a fresh index of the survivors, which is the first.  Ties need no care of their own: both forms break them by row position, and
positions among the survivors order as the old positions do; the cases whose k-th boundary holds a tie are counted and checked
in both forms like the rest."""
import numpy as np
import pytest

from tests import remove_cases as rc

F = np.float32
FLT_MAX = np.finfo(F).max


def both_forms(oracle, metric, Q, X, k, live, labels):
    keep = np.flatnonzero(live)
    a = oracle.search_batch(metric, Q, X[keep], k, ids=None if labels is None else labels[keep], nthreads=8)
    b = oracle.search_batch(metric, Q, X, k, mask=live, ids=labels, nthreads=8)
    return keep, a, b


@pytest.mark.parametrize("case", rc.gpu_cases(), ids=lambda c: c[0])
def test_survivors_alone_equal_every_row_under_the_live_mask(oracle, case):
    tag, shape, removed, with_ids = case
    X, Q0 = rc.corpus(shape)
    n = shape[0]
    live = rc.live_mask(n, removed)
    Q = rc.queries(X, Q0, removed)
    small = shape == rc.SMALL
    Qs, k = (Q[:1], 2048) if small else (Q[:64] if shape == rc.ODD else Q, rc.KS[-1])
    metrics = (rc.L2,) if small or shape == rc.ODD or tag.startswith("overlap") else (rc.L2, rc.COS, rc.DOT)
    labels = rc.ids_for(n) if with_ids else None
    for metric in metrics:
        keep, (ai, ad), (bi, bd) = both_forms(oracle, metric, Qs, X, k, live, labels)
        assert np.array_equal(ad, bd), (tag, metric)
        # without ids the first form reports positions among the survivors: keep[] takes them to the old positions
        a_old = ai if with_ids else np.where(ai >= 0, keep[np.clip(ai, 0, max(keep.size - 1, 0))] if keep.size else -1, -1)
        assert np.array_equal(a_old, bi), (tag, metric)
        nv = int(live.sum())
        assert np.all(bi[:, min(nv, k):] == -1) and np.all(bd[:, min(nv, k):] == FLT_MAX)
        shown = bi[:, :min(nv, k)]
        dead = set((labels[removed] if with_ids else removed).tolist())
        assert not dead.intersection(shown.ravel().tolist()), (tag, metric)
        # ties at the k-th boundary of any k the GPU file asks for: resolved by position in both forms (checked above)
        for kk in ((k,) if small else rc.KS):
            if kk < min(nv, k):
                ties = int((bd[:, kk - 1] == bd[:, kk]).sum())
                assert ties == 0 or np.array_equal(a_old[:, :kk + 1], bi[:, :kk + 1]), (tag, metric, kk, ties)


def test_case_generator_invariants():
    n = rc.MAIN[0]
    assert n - rc.removed_rows(n, "2pct").size >= 0.95 * n
    assert n - rc.removed_rows(n, "18pct").size == 16400
    assert n - rc.removed_rows(n, "60pct").size == 8000
    for name in rc.FRACTIONS:
        r = rc.removed_rows(n, name)
        assert np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < n
    X, Q = rc.corpus(rc.MAIN)
    r = rc.removed_rows(n, "18pct")
    assert np.array_equal(rc.queries(X, Q, r)[0], X[r[len(r) // 2]])
    ids = rc.ids_for(n)
    assert (ids < 0).any() and (ids > 2 ** 32).any()
