"""Sequences of add / filter / remove / compact calls on the code handles that can forget rows, on the GPU, against the model of
tests/lifecycle_model.py: its seeded float32 scripts of about 40 calls (imported, not edited) drive an IVF-PQ handle plain and
residual and an IVF-SQ8 handle.  The model's rows stay what they are; the small adapter below keeps each row's
code beside them (encoded once, when the row is added, and moved by a compaction: never computed again, as on the handle) and
swaps the model's distances for the handle's code oracle (tests/ivf_code_remove_cases.py) over all physical rows with
visible = live & mask.  After every call the return value, the counters, the assignments, the list sizes, the codes and the
searches (k 1, 10 and now and then 64; nprobe 1, 3 and every list; host and device forms in turn) are compared for equality.
After every compaction and at the end a fresh handle filled by add of the survivors' vectors must hold the same codes and answer
alike.  One script per handle runs in the product library and one in the diagnostic library with compaction rounds of
lm.ROUND_ROWS rows.

A failure names the seed, the step and the call, and prints the script up to there, one call per line."""
import numpy as np
import pytest

from tests import ivf_code_remove_cases as cc
from tests import lifecycle_model as lm
from tests.gpu_util import assert_same, diag_lib, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = cc.FLT_MAX
NPROBES = (1, 3, lm.NLIST)
# (with_ids, seed, diagnostic library): seed 1 grows the capacity under a filter at order 1, seed 0 without one at order 0
RUNS = [(False, 1, False), (True, 0, True)]


class CodeModel(lm.Model):
    """lm.Model over float32 rows with the code of each physical row beside it"""

    def __init__(self, oracle, kind, script, par):
        self.k, self.oracle, self.C, self.par, self.order = cc.KINDS[kind], oracle, script.C, par, script.order
        super().__init__("f32", script.dim, script.with_ids, assign=lambda w: self.k.assign(oracle, w, self.C, self.order))
        self.codes = None

    def add(self, rows, ids=None):
        n0 = self.ntotal
        super().add(rows, ids)
        new = self.k.encode(self.oracle, self.wide[n0:], self.C, self.lists[n0:], self.par)  # (a residual code: against the row's list)
        self.codes = new if self.codes is None else np.concatenate([self.codes, new])

    def compact(self):
        keep = np.flatnonzero(self.live)
        self.codes = self.codes[keep]  # the codes move with the rows
        return super().compact()

    def expect(self, Q, k, nprobe):
        """-> (labels, dist, rows scanned per query): the handle's oracle with mask = live & filter"""
        if self.ntotal == 0:  # an empty handle: all padding
            return np.full((Q.shape[0], k), -1, np.int64), np.full((Q.shape[0], k), FLT_MAX, F), np.zeros(Q.shape[0], np.int64)
        return self.k.search(self.oracle, np.asarray(Q, F), self.C, self.lists, self.codes, self.par, self.visible().astype(np.uint8), k,
                             nprobe, ids=self.ids, order=self.order)


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()  # (a copy: the script's arrays are read-only)
    torch.cuda.synchronize()
    return t


def _call(h, op):
    a = op.args
    if op.name == "add":
        return h.add(a["rows"], a.get("ids"))
    if op.name == "reserve":
        return h.reserve(a["n"])
    if op.name == "set_filter":
        return h.set_filter(a["mask"])
    if op.name == "filter_column":
        return h.filter_column(a["column"], a["value"], a["op"], combine=a["combine"])
    if op.name == "remove":
        return h.remove(a["labels"])
    if op.name == "remove_rows":
        return h.remove_rows(a["pos"])
    if op.name == "remove_device":
        d = _dev(a["labels"])
        return h.remove_device(d.numel(), d.data_ptr())
    if op.name == "compact":
        return h.compact()
    raise ValueError(op.name)


def _search(h, Q, k, nprobe, device):
    if not device:
        return h.search(np.asarray(Q, F), k, nprobe)
    import torch
    dQ = _dev(np.asarray(Q, F))
    dD = torch.full((Q.shape[0], k), -5.0, dtype=torch.float32, device="cuda")
    dL = torch.full((Q.shape[0], k), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h.search_device(Q.shape[0], dQ.data_ptr(), k, nprobe, dD.data_ptr(), dL.data_ptr())
    torch.cuda.synchronize()
    return dL.cpu().numpy(), dD.cpu().numpy()


def _ks(op):
    return lm.KS + ((lm.K_PAD,) if op.k64 else ())


def _check_step(m, h, op, got):
    nt, nlive, ndead, nvis = m.counts()
    if op.name in ("remove", "remove_rows", "remove_device", "compact"):
        assert np.array_equal(got["handle"], got["model"]), f"the handle returned {got['handle']}, the model {got['model']}"
    assert cc.counts(h) == (nt, nlive, ndead) and h.nvisible() == nvis, f"the handle's counters {cc.counts(h)} {h.nvisible()}, the model {m.counts()}"
    assert np.array_equal(h.assignments(), m.lists), "assignments"
    assert np.array_equal(h.list_sizes(), np.bincount(m.lists, minlength=lm.NLIST)), "list sizes"
    if nt:
        assert np.array_equal(h.codes(), m.codes), "codes: kept where they are, removed rows included"
    ks = _ks(op)
    forbidden = lm.forbidden_labels(m)
    for nprobe in NPROBES:
        ol, od, scanned = m.expect(op.Q, ks[-1], nprobe)
        for k in ks:
            lab, dist = _search(h, op.Q, k, nprobe, op.device)
            ctx = f"nprobe {nprobe} k {k}"
            assert_same(lab, dist, ol[:, :k], od[:, :k], ctx)
            st = h.last_search_stats()
            assert st[:3] == (lm.NQ, int(scanned.sum()), int(scanned.max())), (st, ctx)
            assert nt == 0 or st[3] == int((scanned <= cc.LDS_KEYS).sum()), (st, ctx)  # (an empty handle launches nothing)
            assert not np.isin(lab, forbidden).any(), f"{ctx}: a removed or hidden row came back"


def _check_fresh(kind, s, m, h, op, lib):
    """a fresh handle filled by add of the survivors' vectors, their ids and the mask restricted to them: the same codes, the same
    answers"""
    keep, rows, _, ids, mask, lists = m.survivors()
    h2 = cc.KINDS[kind].handle(s.C, m.par, order=s.order, lib=lib)
    try:
        if keep.size:
            h2.add(rows, ids)
            if mask is not None:
                h2.set_filter(mask)
            assert np.array_equal(h2.codes(), m.codes[keep]), "the survivors' vectors encode to the codes the handle kept"
        ks = _ks(op)
        Q = np.asarray(op.Q, F)
        if m.counts()[2] == 0:
            if keep.size:
                cc.same_handles(h, h2, Q, "a fresh handle of the survivors", ks=ks, nprobes=NPROBES)
            return
        # (the end of a script that holds removed rows: positions and lists still count them)
        back = (lambda lab: lab) if s.with_ids else (lambda lab: cc.back(lab, keep))
        assert h.nvisible() == h2.nvisible() and np.array_equal(h2.assignments(), lists)
        for nprobe in NPROBES:
            for k in ks:
                lab, dist = h.search(Q, k, nprobe)
                l2, d2 = h2.search(Q, k, nprobe)
                assert_same(lab, dist, back(l2), d2, f"a fresh handle of the survivors, nprobe {nprobe} k {k}")
                assert h.last_search_stats() == h2.last_search_stats()
    finally:
        h2.Close()


@pytest.mark.parametrize("with_ids,seed,diag", RUNS, ids=["product", "diagnostic rounds of 7"])
@pytest.mark.parametrize("kind", list(cc.KINDS))
def test_code_lifecycle(oracle, kind, with_ids, seed, diag):
    lib = diag_lib() if diag else gpu_or_skip()
    s = lm.script(seed, "f32", with_ids)
    par = cc.KINDS[kind].small_case(s.dim, seed)
    m = CodeModel(oracle, kind, s, par)
    h = cc.KINDS[kind].handle(s.C, par, order=s.order, lib=lib)
    if diag:
        lib.lb_debug_set_compact_round_rows(lm.ROUND_ROWS)
    try:
        for step, op in enumerate(s.ops):
            try:
                got = {"handle": _call(h, op), "model": lm.apply(m, op)}
                _check_step(m, h, op, got)
                if op.name == "compact" or step == len(s.ops) - 1:
                    _check_fresh(kind, s, m, h, op, lib)
            except Exception as e:
                raise AssertionError(f"{kind} seed {seed} ids {with_ids} (order {s.order} dim {s.dim}"
                                     f"{', compaction rounds of 7 rows' if diag else ''}) step {step}: {op}\n"
                                     f"  {type(e).__name__}: {e}\n  model counts {m.counts()} filter {'on' if m.mask is not None else 'off'}"
                                     f" {'device' if op.device else 'host'} forms\nthe script up to there:\n{s.prefix(step)}") from e
    finally:
        if diag:
            lib.lb_debug_set_compact_round_rows(0)
        h.Close()
