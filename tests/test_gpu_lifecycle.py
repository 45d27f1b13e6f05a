"""Sequences of add / filter / remove / compact calls on the GPU, against a model (tests/lifecycle_model.py): a flat index
(lb_gpu_index_*) and an IVF-Flat handle (lb_gpu_ivf_*) are driven through the same seeded script of about 40 calls, float32,
float16 and int8 rows, with ids and without.  After every call the return value, the counters, the IVF handle's assignments and
list sizes and the searches of both handles (k 1, 10 and now and then 64; nprobe 1, 3 and every list; host and device forms in
turn) are compared for equality with the model's: the oracle over all physical rows with visible = live & mask, which
tests/test_lifecycle_model_semantics.py pins on the CPU to the header's "a fresh index holding only the live rows".  The IVF
handle with every list probed must answer as the flat index does.  After every compaction and at the end fresh handles of the
survivors must answer alike.  One script per element type runs in the diagnostic library with compaction rounds of 7 rows.

A failure names the seed, the step and the call, and prints the script up to there, one call per line."""
import numpy as np
import pytest

from tests import ivf_remove_cases as vc
from tests import lifecycle_model as lm
from tests import refine_oracle
from tests.gpu_util import assert_same, diag_lib, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(F).max
NPROBES = (1, 3, lm.NLIST)


def _handles(kind, dim, metric, order, C_, lib):
    from longbow_amd import gpu, ivf
    dt = {"f32": gpu.DataType.Float32, "f16": gpu.DataType.Float16, "i8": gpu.DataType.Int8}[kind]
    flat = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=dim, Metric=metric, DataType=dt), lib=lib)
    try:
        if kind != "i8":  # (the int8 kernels have one order; an int8 IVF handle's order is its coarse index's)
            flat.set_order(order)
        h = ivf.IVFFlatInt8(C_, metric, order, lib=lib) if kind == "i8" else ivf.IVFFlat(C_, metric, order, lib=lib, dtype=dt)
    except Exception:
        flat.Close()
        raise
    return flat, h


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()  # (a copy: the script's arrays are read-only)
    torch.cuda.synchronize()
    return t


def _call(flat, h, op):
    """the step on both handles -> what each returned; the two filter_column signatures differ, the test adapts"""
    a = op.args
    if op.name == "add":
        return flat.Add(a.get("ids"), a["rows"]), h.add(a["rows"], a.get("ids"))
    if op.name == "reserve":
        return flat.reserve(a["n"]), h.reserve(a["n"])
    if op.name == "set_filter":
        return flat.set_filter(a["mask"]), h.set_filter(a["mask"])
    if op.name == "filter_column":
        return (flat.filter_column(a["column"], a["op"], a["value"], combine=a["combine"]),
                h.filter_column(a["column"], a["value"], a["op"], combine=a["combine"]))
    if op.name == "remove":
        return flat.Remove(a["labels"]), h.remove(a["labels"])
    if op.name == "remove_rows":
        return flat.remove_rows(a["pos"]), h.remove_rows(a["pos"])
    if op.name == "remove_device":
        d = _dev(a["labels"])
        return flat.remove_device(d.numel(), d.data_ptr()), h.remove_device(d.numel(), d.data_ptr())
    if op.name == "compact":
        return flat.Compact(), h.compact()
    raise ValueError(op.name)


def _ivf_queries(kind, Q):
    return Q if kind == "i8" else np.asarray(Q, F)  # (a float16 handle takes f32 queries: float16 ones widened, which is exact)


def _search(kind, flat, h, Q, k, nprobe, device):
    """-> (labels, dist) of the flat index (nprobe None) or of the IVF handle, by the host form or the device-pointer form"""
    if not device:
        return flat.SearchBatch(Q, k) if nprobe is None else h.search(_ivf_queries(kind, Q), k, nprobe)
    import torch
    dQ = _dev(Q if nprobe is None else _ivf_queries(kind, Q))
    dD = torch.full((Q.shape[0], k), -5.0, dtype=torch.float32, device="cuda")
    dL = torch.full((Q.shape[0], k), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    if nprobe is None:
        flat.search_device(Q.shape[0], dQ.data_ptr(), k, dD.data_ptr(), dL.data_ptr())
    else:
        h.search_device(Q.shape[0], dQ.data_ptr(), k, nprobe, dD.data_ptr(), dL.data_ptr())
    torch.cuda.synchronize()
    return dL.cpu().numpy(), dD.cpu().numpy()


def _ks(op):
    return lm.KS + ((lm.K_PAD,) if op.k64 else ())


def _check_step(oracle, s, m, flat, h, op, ret):
    kind, metric, order = s.kind, s.metric, s.order
    nt, nlive, ndead, nvis = m.counts()
    # return values
    if op.name in ("remove", "remove_rows", "remove_device", "compact"):
        want = ret["model"]
        for who, got in (("flat", ret["flat"]), ("ivf", ret["ivf"])):
            assert np.array_equal(got, want), f"{who} returned {got}, the model {want}"
    # counters, assignments
    assert (flat.ntotal, flat.nlive(), flat.ndeleted()) == (nt, nlive, ndead), "the flat index's counters"
    assert vc.counts(h) == (nt, nlive, ndead) and h.nvisible() == nvis, f"the IVF handle's counters {vc.counts(h)} {h.nvisible()}, the model {m.counts()}"
    assert np.array_equal(h.assignments(), m.lists), "assignments"
    assert np.array_equal(h.list_sizes(), np.bincount(m.lists, minlength=lm.NLIST)), "list sizes"
    # searches
    ks = _ks(op)
    forbidden = lm.forbidden_labels(m)
    planted = metric == 0 and nvis > 0  # query 1 is a visible row's own vector
    fl, fd = lm.expect_flat(oracle, m, metric, order, op.Q, ks[-1])
    flat_got = {}
    for k in ks:
        lab, dist = flat_got[k] = _search(kind, flat, h, op.Q, k, None, op.device)
        assert_same(lab, dist, fl[:, :k], fd[:, :k], f"flat k {k}")
        assert not np.isin(lab, forbidden).any(), f"flat k {k}: a removed or hidden row came back"
        assert not planted or dist[1, 0] == 0, f"flat k {k}: the planted row is not first"
    for nprobe in NPROBES:
        ol, od, scanned = lm.expect_ivf(oracle, m, metric, order, op.Q, s.C, ks[-1], nprobe)
        for k in ks:
            lab, dist = _search(kind, flat, h, op.Q, k, nprobe, op.device)
            ctx = f"ivf nprobe {nprobe} k {k}"
            assert_same(lab, dist, ol[:, :k], od[:, :k], ctx)
            st = h.last_search_stats()
            assert st[:3] == (lm.NQ, int(scanned.sum()), int(scanned.max())), (st, ctx)
            assert nt == 0 or st[3] == int((scanned <= vc.LDS_KEYS).sum()), (st, ctx)  # (an empty handle launches nothing)
            assert not np.isin(lab, forbidden).any(), f"{ctx}: a removed or hidden row came back"
            assert not planted or dist[1, 0] == 0, f"{ctx}: the planted row is not first"
            if nprobe == lm.NLIST:  # the differential the header promises
                assert_same(lab, dist, *flat_got[k], f"{ctx} against the flat index")
    # refine and rerank over positions that include removed ones
    if op.short is not None and kind != "i8" and nt:
        Qf = np.asarray(op.Q, F)
        dead = np.flatnonzero(m.live == 0)
        scrubbed = np.where(np.isin(op.short, dead), -1, op.short)
        lab, dist = flat.Refine(Qf, op.short, 10)
        wl, wd = refine_oracle.refine(oracle, metric, Qf, m.wide, scrubbed, 10, order, ids=m.ids)
        assert_same(lab, dist, wl, wd, "Refine: removed positions join the padding")
        assert not np.isin(lab, np.setdiff1d(m.labels()[dead], m.labels()[m.live != 0])).any(), "Refine returned a removed row"
    if op.short is not None and kind == "f32" and nt:  # (re-rank reads float32 rows: a float16 index refuses it)
        Qf = np.asarray(op.Q, F)
        rows = op.short[0]
        inside = rows >= 0
        want = np.full(rows.size, FLT_MAX, F)
        want[inside] = oracle.batch_flat(metric, Qf[0], m.wide[rows[inside]], order)
        got = flat.Rerank(Qf[0], rows, order=order, want_score=False)
        assert np.array_equal(got, want), "Rerank: a distance for every position, removed or not"


def _check_fresh(s, m, flat, h, op, lib):
    """fresh handles of the survivors, their ids and the mask restricted to them answer as the handles do"""
    keep, rows, _, ids, mask, lists = m.survivors()
    f2, h2 = _handles(s.kind, s.dim, s.metric, s.order, s.C, lib)
    try:
        if keep.size:
            f2.Add(ids, rows)
            h2.add(rows, ids)
            if mask is not None:
                f2.set_filter(mask)
                h2.set_filter(mask)
        back = (lambda lab: lab) if s.with_ids else (lambda lab: np.where(lab >= 0, np.append(keep, -1)[np.clip(lab, 0, None)], -1))
        ks = _ks(op)
        for k in ks:
            lab, dist = flat.SearchBatch(op.Q, k)
            l2, d2 = f2.SearchBatch(op.Q, k)
            assert_same(lab, dist, back(l2), d2, f"a fresh flat index of the survivors, k {k}")
        Qi = _ivf_queries(s.kind, op.Q)
        if m.counts()[2] == 0:
            vc.same_handles(h, h2, Qi, "a fresh IVF handle of the survivors", ks=ks, nprobes=NPROBES)
        else:  # (the end of a script that holds removed rows: positions and lists still count them)
            assert h.nvisible() == h2.nvisible() and np.array_equal(h2.assignments(), lists) and np.array_equal(h.assignments(), m.lists)
            for nprobe in NPROBES:
                for k in ks:
                    lab, dist = h.search(Qi, k, nprobe)
                    l2, d2 = h2.search(Qi, k, nprobe)
                    assert_same(lab, dist, back(l2), d2, f"a fresh IVF handle of the survivors, nprobe {nprobe} k {k}")
                    assert h.last_search_stats() == h2.last_search_stats()
    finally:
        f2.Close()
        h2.Close()


@pytest.mark.parametrize("kind,with_ids,seed", lm.PARAMS)
def test_lifecycle(oracle, kind, with_ids, seed):
    diag = (kind, with_ids, seed) in lm.DIAG
    lib = diag_lib() if diag else gpu_or_skip()
    s = lm.script(seed, kind, with_ids)
    m = lm.Model(kind, s.dim, with_ids, assign=lm.assigner(oracle, s.metric, s.order, s.C))
    flat, h = _handles(kind, s.dim, s.metric, s.order, s.C, lib)
    if diag:
        lib.lb_debug_set_compact_round_rows(lm.ROUND_ROWS)
    try:
        for step, op in enumerate(s.ops):
            try:
                got = _call(flat, h, op)
                ret = {"model": lm.apply(m, op), "flat": got[0], "ivf": got[1]}
                _check_step(oracle, s, m, flat, h, op, ret)
                if op.name == "compact" or step == len(s.ops) - 1:
                    _check_fresh(s, m, flat, h, op, lib)
            except Exception as e:
                raise AssertionError(f"seed {seed} {kind} ids {with_ids} (metric {s.metric} order {s.order} dim {s.dim}"
                                     f"{', compaction rounds of 7 rows' if diag else ''}) step {step}: {op}\n"
                                     f"  {type(e).__name__}: {e}\n  model counts {m.counts()} filter {'on' if m.mask is not None else 'off'}"
                                     f" {'device' if op.device else 'host'} forms\nthe script up to there:\n{s.prefix(step)}") from e
    finally:
        if diag:
            lib.lb_debug_set_compact_round_rows(0)
        flat.Close()
        h.Close()
