"""tests/lifecycle_model.py pinned to include/longbow_gpu.h on the CPU, with the oracle alone, for every (kind, with_ids, seed) that
tests/test_gpu_lifecycle.py runs (lifecycle_model.PARAMS, the one list both files read):

- after every step of every script the model's expected search -- the oracle over all physical rows with visible = live & mask,
  which is what the GPU file compares the handles with -- IS the oracle's search of a fresh corpus of the survivors alone, with
  ids = the old labels and the mask restricted to them ("bit for bit what a fresh index holding only the live rows ... would
  answer"); without ids the fresh corpus labels by position, and the survivors' positions take them back.  Flat and IVF, the
  identity tests/test_ivf_remove_semantics.py pins for one removal, here for sequences;
- the rows a sequence of compactions leaves are the rows the accumulated old_rows name;
- the scripts are deterministic and each meets the coverage conditions its seed is drawn for, with the oracle's lists."""
import numpy as np
import pytest

from tests import i8_oracle
from tests import ivf_i8_oracle as o8
from tests import ivf_oracle as io
from tests import lifecycle_model as lm

F = np.float32
NPROBES = (1, 3, lm.NLIST)


def _back(labels, keep):
    return np.where(labels >= 0, np.append(keep, -1)[np.clip(labels, 0, None)], -1)  # (appended: no survivors, all padding)


def _fresh_flat(oracle, s, Q, rows, wide, ids, mask, k):
    if s.kind == "i8":
        vis = None if mask is None else np.flatnonzero(mask)
        return i8_oracle.search(s.metric, Q, rows, k, ids=ids, visible=vis)
    return oracle.search_batch(s.metric, np.asarray(Q, F), wide, k, order=s.order, mask=mask, ids=ids, nthreads=8)


def _fresh_ivf(oracle, s, Q, rows, wide, ids, mask, lists, k, nprobe):
    ids = ids if rows.shape[0] else None  # (no survivors: all padding, and no id to look up)
    if s.kind == "i8":
        return o8.search(oracle, s.metric, s.order, Q, rows, s.C, lists, k, nprobe, ids=ids, mask=mask)
    hidden = lists if mask is None else np.where(mask != 0, lists, -1)
    return io.search(oracle, s.metric, s.order, np.asarray(Q, F), wide, s.C, hidden, k, nprobe, ids=ids)


@pytest.mark.parametrize("kind,with_ids,seed", lm.PARAMS)
def test_the_model_is_the_fresh_corpus_of_the_survivors(oracle, kind, with_ids, seed):
    s = lm.script(seed, kind, with_ids)
    m = lm.Model(kind, s.dim, with_ids, assign=lm.assigner(oracle, s.metric, s.order, s.C))
    every = np.empty((0, s.dim), F)          # every row ever added, in the order of the adds
    origin = np.empty(0, np.int64)           # which of them each physical row is, through the accumulated old_rows
    lists_per_step = []
    for step, op in enumerate(s.ops):
        ctx = f"seed {seed} {kind} ids {with_ids} step {step} {op}"
        ret = lm.apply(m, op)
        if op.name == "add":
            n = op.args["rows"].shape[0]
            origin = np.concatenate([origin, np.arange(every.shape[0], every.shape[0] + n)])
            every = np.concatenate([every, lm.widen(kind, op.args["rows"])])
        if op.name == "compact":
            assert np.all(np.diff(ret) > 0) and ret.size == m.ntotal, ctx
            origin = origin[ret]
        assert np.array_equal(m.wide, every[origin]), ctx
        lists_per_step.append(m.lists.copy())
        keep, rows, wide, ids, mask, lists = m.survivors()
        k = lm.K_PAD if op.k64 else lm.KS[-1]
        ml, md = lm.expect_flat(oracle, m, s.metric, s.order, op.Q, k)
        fl, fd = _fresh_flat(oracle, s, op.Q, rows, wide, ids, mask, k)
        assert np.array_equal(ml, fl if with_ids else _back(fl, keep)) and np.array_equal(md, fd), ctx
        assert not np.isin(ml, lm.forbidden_labels(m)).any(), ctx
        for nprobe in NPROBES:
            ml, md, ms = lm.expect_ivf(oracle, m, s.metric, s.order, op.Q, s.C, k, nprobe)
            fl, fd, fs = _fresh_ivf(oracle, s, op.Q, rows, wide, ids, mask, lists, k, nprobe)
            assert np.array_equal(ml, fl if with_ids else _back(fl, keep)) and np.array_equal(md, fd) and np.array_equal(ms, fs), (ctx, nprobe)
            if nprobe == lm.NLIST:  # every list probed: the flat index's answer, and every visible row scanned
                pl, pd = lm.expect_flat(oracle, m, s.metric, s.order, op.Q, k)
                assert np.array_equal(ml, pl) and np.array_equal(md, pd) and (ms == m.counts()[3]).all(), ctx
    # the coverage conditions, with the oracle's lists in place of the generator's float64 ones
    cov = lm.coverage(s, lists_per_step)
    assert lm.missing(s, cov) == [], (kind, with_ids, seed)


def test_scripts_are_deterministic():
    for kind, with_ids, seed in lm.PARAMS[::4]:
        a = lm.script(seed, kind, with_ids)
        b = lm.script.__wrapped__(seed, kind, with_ids)
        assert a is not b and len(a.ops) == len(b.ops) and a.attempt == b.attempt and np.array_equal(a.C, b.C)
        for x, y in zip(a.ops, b.ops):
            assert x.name == y.name and x.k64 == y.k64 and x.device == y.device and np.array_equal(x.Q, y.Q)
            assert (x.short is None) == (y.short is None) and (x.short is None or np.array_equal(x.short, y.short))
            assert x.args.keys() == y.args.keys()
            for key in x.args:
                assert np.array_equal(x.args[key], y.args[key]) if isinstance(x.args[key], np.ndarray) else x.args[key] == y.args[key]
    assert lm.script(1, "f16", True).ops[3].name != "" and len({str(lm.script(s, "f32", False).ops[1]) for s in lm.SEEDS}) > 1


def test_what_the_scripts_cover_between_them():
    """per (kind, with_ids), across its seeds: every state of the list (the one about ids with ids only, the one about renumbering
    without), both kinds of capacity growth over removed rows, every kind of compaction, every metric the kind takes, both orders
    for f32, and the 28-byte rows once"""
    for kind in lm.KINDS:
        for with_ids in (False, True):
            covs = [lm.coverage(lm.script(seed, kind, with_ids)) for seed in lm.SEEDS]
            states = set().union(*(c["states"] for c in covs))
            assert states == set(lm.STATES) - {lm.NO_IDS_ONLY if with_ids else lm.IDS_ONLY}, (kind, with_ids)
            grow = set().union(*(c["grow"] for c in covs))
            assert {("flat", False), ("ivf", False), ("flat", True), ("ivf", True)} <= grow, (kind, with_ids)
            for c in covs:
                assert c["compact"] == {"filter", "no filter", "nothing removed", "empty then add"}
                assert set(lm.MUTATING) <= c["ops"]
        metrics = {lm.shape_of(kind, False, seed)[1] for seed in lm.SEEDS}
        assert metrics == ({0, 2} if kind == "i8" else {0, 1, 2})
    assert {lm.shape_of("f32", False, seed)[2] for seed in lm.SEEDS} == {0, 1}
    assert [lm.shape_of(*p)[0] for p in lm.PARAMS].count(7) == 1
    assert len(lm.PARAMS) == 18 and all(sum(p[0] == kind for p in lm.DIAG) == 1 for kind in lm.KINDS)


def test_the_removal_methods_ignore_what_the_header_lists():
    m = lm.Model("f32", 4, True)
    m.add(np.arange(24, dtype=F).reshape(6, 4), np.array([10, 20, 30, 20, 50, 60]))
    assert m.remove([20, 20, -1, 999]) == 2 and m.counts() == (6, 4, 2, 4)  # both rows under one id; a repeat, -1, an unknown id
    assert m.remove([20]) == 0 and m.remove_rows([1, 3, -1, 6, 11, -2 ** 40]) == 0  # rows already removed; outside [0, ntotal)
    assert m.remove_rows([0, 0, 5]) == 2 and m.remove_device([30]) == 1
    m.set_filter(np.array([1, 1, 1, 1, 0x80, 1], np.uint8))
    assert np.array_equal(m.compact(), [4]) and m.counts() == (1, 1, 0, 1) and m.mask.tolist() == [0x80] and m.ids.tolist() == [50]
    m.filter_column(np.array([7], np.int64), lm.rv.GE, 7, combine=True)  # bytewise, as simd.AndBytes: 0x80 AND 1 is 0
    assert m.counts() == (1, 1, 0, 0)
    n = lm.Model("i8", 4, False)
    n.add(np.zeros((5, 4), np.int8))
    assert n.remove([1, 3]) == 2 and np.array_equal(n.compact(), [0, 2, 4])
    assert n.remove([1, 3]) == 1 and n.labels().tolist() == [0, 1, 2]          # renumbered: label 1 is the old row 2; 3 names no row
    assert (lm.flat_capacity(0, 1200), lm.flat_capacity(1200, 1201), lm.ivf_capacity(0, 1), lm.ivf_capacity(4096, 4097)) == (1200, 2400, 4096, 8192)
