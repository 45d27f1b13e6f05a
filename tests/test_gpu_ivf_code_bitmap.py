"""A row bitmap given with the search call on the IVF-PQ handle plain ("pq") and residual ("rpq") and on the IVF-SQ8 handle ("sq8")
(lb_gpu_ivfpq_search_bitmap_ctx / _bitmap_device_ctx, lb_gpu_ivfsq8_search_bitmap_ctx / _bitmap_device_ctx) on the GPU.  The
expected result everywhere is the kind's oracle with mask = bits & filter & live (tests/ivf_code_bitmap_cases.py, pinned on the CPU
by tests/test_ivf_code_bitmap_semantics.py); labels and distances are compared for equality and last_search_stats shows that the
search walked the passing rows alone.  The shapes are the smallest at which the compaction of the probed lists can go wrong in any
of its forms: lists of rows (sq8), of positions over all rows (pq, rpq without a filter) and of positions behind a visible list
(pq, rpq with a filter or removed rows); one compaction per (query, probe slot) and one per call (the host's rule, restated in
ivf_code_bitmap_cases.shared_form: each test says which side its shapes are on); list lengths and kept counts around the
compaction's 2048-position step and each scan's tile; lists emptied by the bitmap; the selection's 16,384 LDS keys under an
unfiltered bound beyond them; more lists than a wave has lanes, than LB_MAX_K, than rows; bitmaps at odd addresses with ones behind
their last bit."""
import threading

import numpy as np
import pytest

from tests import ivf_bitmap_cases as bc
from tests import ivf_code_bitmap_cases as kc
from tests import ivf_code_remove_cases as cc
from tests import ivf_filter_cases as fc
from tests import ivf_i8_oracle as o8
from tests import ivf_oracle as io
from tests import refine_oracle as fo
from tests.gpu_util import assert_same, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
OK, INVALID, CANCELLED = 0, 1, 8
K = kc.K
KINDS = list(cc.KINDS)
FLT_MAX = cc.FLT_MAX
LB_MAX_K = 2048


def _handle(c, rows=None, ids=None):
    """a handle of the case's kind holding its rows (`rows`: those positions alone, in that order)"""
    h = c.k.handle(c.C, c.par, lib=gpu_or_skip())
    X = c.X if rows is None else c.X[rows]
    if X.shape[0]:
        h.add(X, ids)
    return h


def _stats(scanned, nq):
    return (nq, int(scanned.sum()), int(scanned.max()), int((scanned <= fc.LDS_KEYS).sum()))


def _check(oracle, c, h, Q, mask, ks, nprobe, also=None, ids=None, rows=None, ctx=""):
    """labels, distances and all four counters of the searches under the bitmap of `mask` at every k of ks against one oracle call
    at the largest (a smaller k's answer is its prefix) -> rows scanned per query"""
    bits = bc.pack(mask)
    ol, od, scanned = kc.search_bitmap(oracle, c, Q, bits, max(ks), nprobe, also=also, ids=ids, rows=rows)
    for k in ks:
        lab, dist = h.search(Q, k, nprobe, bitmap=bits)
        assert_same(lab, dist, ol[:, :k], od[:, :k], f"{ctx} k {k}")
        assert h.last_search_stats() == _stats(scanned, Q.shape[0]), (h.last_search_stats(), scanned.sum(), scanned.max(), ctx, k)
    return scanned


def _shared(h, nq, nprobe, stride=0, sizes=None):
    return kc.shared_form(h.list_sizes() if sizes is None else sizes, nq, nprobe, stride)


def _first(oracle, kind):
    return cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", cc.SHAPES, ids=cc.SHAPE_IDS)
def test_parity_under_every_mask_as_a_bitmap(oracle, kind, shape):
    c = cc.parity(oracle, kind, shape)
    h = _handle(c)
    try:
        plain = {nprobe: (h.search(c.Q, K, nprobe), h.last_search_stats()) for nprobe in (1, 3, 16)}
        masks = fc.parity_masks()
        names = list(masks) if shape == cc.FIRST_SHAPE[kind] else ["10 % byte mask", "50 % byte mask"]
        for name in names:
            for nprobe in (1, 3, 16):
                _check(oracle, c, h, c.Q, masks[name], (10, 100), nprobe, ctx=f"{kind} {shape} {name} nprobe {nprobe}")
                # the handle is what it was: no filter on it, and the plain search answers as before
                assert h.nvisible() == h.ntotal == c.n
                assert_same(*h.search(c.Q, K, nprobe), *plain[nprobe][0], f"plain search after {name}")
                assert h.last_search_stats() == plain[nprobe][1]
    finally:
        h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_equal_to_the_same_handle_under_set_filter(oracle, kind):
    c = _first(oracle, kind)
    h = _handle(c, ids=cc.ids_for(c.n)) if kind == "pq" else _handle(c)  # (one kind with ids: the labels are those)
    masks = fc.parity_masks()
    try:
        for name in ("10 % byte mask", "50 % byte mask", "row 0", "all-zero", "all-one"):
            bits = bc.pack(masks[name])
            got = {(nprobe, k): (h.search(c.Q, k, nprobe, bitmap=bits), h.last_search_stats()) for nprobe in (1, 3, 16) for k in (10, 100)}
            assert h.nvisible() == c.n
            h.set_filter(masks[name])
            for (nprobe, k), ((lab, dist), st) in got.items():
                assert_same(lab, dist, *h.search(c.Q, k, nprobe), f"{kind} {name} nprobe {nprobe} k {k}")
                assert st == h.last_search_stats(), (kind, name, nprobe, k)
            h.set_filter(None)
    finally:
        h.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
def _edges(oracle, c, h, keep, mask, ctx):
    """the whole batch at one and two probes (one compaction per call: its queries times the longest list exceed the rows), then
    each of the first nlist queries alone (one compaction per probe slot: one list is fewer rows than all) -> the batch's labels"""
    nl = c.nlist
    reps = c.Q.shape[0] // nl  # query i probes list i % nlist first
    sizes = np.bincount(c.lists, minlength=nl)
    bits = bc.pack(mask)
    assert kc.shared_form(sizes, c.Q.shape[0], 1, 0) and kc.shared_form(sizes, nl, 2, 0) and not kc.shared_form(sizes, 1, 1, 0)
    scanned = _check(oracle, c, h, c.Q, mask, (10, 200), 1, ctx=f"{ctx} nprobe 1")
    assert scanned.tolist() == list(keep) * reps
    _check(oracle, c, h, c.Q[:nl], mask, (10, 200), 2, ctx=f"{ctx} nprobe 2")
    lab, dist = h.search(c.Q, 10, 1, bitmap=bits)
    for q in range(nl):
        l1, d1 = h.search(c.Q[q:q + 1], 10, 1, bitmap=bits)
        assert_same(l1, d1, lab[q:q + 1], dist[q:q + 1], f"{ctx} query {q} alone")
        assert h.last_search_stats() == (1, keep[q], keep[q], 1)
    for l in np.flatnonzero(np.asarray(keep) == 0):  # a probed list with no set bit, emptied or empty: all padding
        assert (lab[l] == -1).all() and (dist[l] == FLT_MAX).all()
    assert h.list_sizes().tolist() == sizes.tolist() and h.nvisible() == c.n
    return lab, dist


@pytest.mark.parametrize("choice", ["first rows", "random rows"])
@pytest.mark.parametrize("kind", KINDS)
def test_kept_counts_at_the_edges_of_the_compaction_step(oracle, kind, choice):
    c = kc.step_case(oracle, kind)
    mask = fc.keep_per_list(c.lists, bc.STEP_KEEP, None if choice == "first rows" else np.random.default_rng(6))
    h = _handle(c)
    try:
        assert h.list_sizes().tolist() == list(bc.STEP_COUNTS)
        lab, dist = _edges(oracle, c, h, bc.STEP_KEEP, mask, f"{kind} step {choice}")
        assert lab[1, 0] == np.flatnonzero((c.lists == 1) & (mask != 0))[0] and (lab[1, 1:] == -1).all() and (dist[1, 1:] == FLT_MAX).all()
    finally:
        h.Close()


@pytest.mark.parametrize("choice", ["first rows", "random rows"])
@pytest.mark.parametrize("keeps", ["A", "B"])
@pytest.mark.parametrize("kind", KINDS)
def test_kept_counts_at_the_edges_of_the_scan_tile(oracle, kind, keeps, choice):
    c = cc.edge(oracle, kind)
    keep = cc.edge_keeps(kind)[keeps]
    mask = fc.keep_per_list(c.lists, keep, None if choice == "first rows" else np.random.default_rng(6))
    h = _handle(c)
    try:
        _edges(oracle, c, h, keep, mask, f"{kind} {keeps} {choice}")
    finally:
        h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_selection_follows_the_kept_count_not_the_bound(oracle, kind):
    """list 0 holds about 37,000 rows, so pmax, which stays the unfiltered bound, is beyond every selection from LDS; with exactly
    16,384 of its bits set the queries that probe it are selected from LDS, with one more they are not.  8 queries x 1 probe under
    one bitmap: 8 x 37,000 exceeds the 50,000 rows, so every list is compacted once for the call, a list of 37,000 rows among them"""
    c = cc.skew(oracle, kind)
    sizes = np.bincount(c.lists, minlength=c.nlist)
    assert sizes[0] > 2 * fc.LDS_KEYS and c.Q.shape[0] == 8 and kc.shared_form(sizes, 8, 1, 0)
    on0 = int((np.array([io.probes(oracle, 0, 0, q, c.C, 1)[0] for q in c.Q]) == 0).sum())
    assert 0 < on0 < 8
    h = _handle(c)
    try:
        for keep0, from_lds in ((fc.LDS_KEYS, 8), (fc.LDS_KEYS + 1, 8 - on0)):
            mask = fc.skew_mask(c.lists, keep0)
            _check(oracle, c, h, c.Q, mask, (10, 100), 1, ctx=f"{kind}: {keep0} bits set in list 0")
            assert h.last_search_stats()[3] == from_lds and h.last_search_stats()[2] == keep0
    finally:
        h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_both_placements_of_the_compaction(oracle, kind):
    c = _first(oracle, kind)
    n, nq = c.n, c.Q.shape[0]
    mask = fc.parity_masks()["50 % byte mask"]
    h = _handle(c)
    try:
        # one query x one probe walks at most the largest list, fewer rows than the handle holds: a compaction per probe slot
        assert not _shared(h, 1, 1)
        for q in (0, 7, 32):
            _check(oracle, c, h, c.Q[q:q + 1], mask, (10, 100), 1, ctx=f"{kind} query {q} alone, one probe")
        # 33 queries x 16 probes would walk 33 x 3,000 list positions of 3,000 rows: every list once for the call
        assert _shared(h, nq, 16)
        _check(oracle, c, h, c.Q, mask, (10, 100), 16, ctx=f"{kind} 33 queries, 16 probes")
        # the same mask 33 times with a stride is a bitmap per query, hence a compaction per slot; at stride 0 it is the shared form
        rows = bc.pack_rows(np.broadcast_to((mask != 0).astype(np.uint8), (nq, n)))
        for nprobe in (1, 3, 16):
            assert not _shared(h, nq, nprobe, stride=bc.nbytes(n)) and _shared(h, nq, nprobe)
            a = h.search(c.Q, K, nprobe, bitmap=rows, bitmap_stride=bc.nbytes(n))
            sa = h.last_search_stats()
            b = h.search(c.Q, K, nprobe, bitmap=rows[0])
            assert_same(*a, *b, f"{kind}: 33 equal bitmaps against one, nprobe {nprobe}")
            assert sa == h.last_search_stats()
    finally:
        h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_bitmap_per_query(oracle, kind):
    c = _first(oracle, kind)
    n, nq = c.n, c.Q.shape[0]
    masks = bc.per_query_masks(nq, n)
    stride = bc.nbytes(n) + 5
    bits = bc.pack_rows(masks, stride=stride, fill=0xFF)
    h = _handle(c)
    try:
        for nprobe in (1, 3, 16):
            lab, dist = h.search(c.Q, K, nprobe, bitmap=bits, bitmap_stride=stride)
            st = h.last_search_stats()
            scanned = np.empty(nq, np.int64)
            for q in range(nq):  # each row is the single-bitmap search of that query: on the GPU, and at three probes in the oracle
                l1, d1 = h.search(c.Q[q:q + 1], K, nprobe, bitmap=bits[q, :bc.nbytes(n)])
                assert_same(lab[q:q + 1], dist[q:q + 1], l1, d1, f"{kind} nprobe {nprobe} query {q}")
                scanned[q] = h.last_search_stats()[1]
            assert st == _stats(scanned, nq)
            assert (lab[0] == -1).all() and scanned[0] == 0                   # the all-zero bitmap
            if nprobe == 3:
                ol, od, osc = kc.search_strided(oracle, c, c.Q, bits, K, nprobe)
                assert_same(lab, dist, ol, od, f"{kind} stride {stride} against the oracle")
                assert np.array_equal(scanned, osc)
        import longbow_amd.ivfpq as mp
        import longbow_amd.ivfsq8 as ms
        pb, ps = (ms if kind == "sq8" else mp).pack_bitmap(masks)
        assert_same(*h.search(c.Q, K, 3, bitmap=pb, bitmap_stride=ps), *h.search(c.Q, K, 3, bitmap=bits, bitmap_stride=stride), "pack_bitmap")
    finally:
        h.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_and_with_the_handle_filter_and_with_removed_rows(oracle, kind):
    """on pq and rpq the handle then walks visible lists of positions, and the compaction looks the bit up through the row at each"""
    c = _first(oracle, kind)
    n = c.n
    rng = np.random.default_rng(21)
    hmask = (fc.parity_masks()["50 % byte mask"] != 0).astype(np.uint8)
    gone = np.sort(rng.permutation(n)[:n // 10])
    live = cc.live_mask(n, gone)
    call = (rng.random(n) < 0.5).astype(np.uint8)
    h = _handle(c)
    try:
        h.set_filter(hmask)
        assert h.remove_rows(gone) == gone.size
        nvis = h.nvisible()
        assert nvis == np.count_nonzero(hmask & live)
        for nprobe in (1, 3, 16):
            scanned = _check(oracle, c, h, c.Q, call, (10, 100), nprobe, also=hmask & live, ctx=f"{kind}: filter AND live AND bitmap, nprobe {nprobe}")
            assert scanned.sum() < c.search(oracle, c.Q, hmask & live, K, nprobe)[2].sum()
            _check(oracle, c, h, c.Q[5:6], call, (10,), nprobe, also=hmask & live, ctx=f"{kind}: one query, nprobe {nprobe}")  # (per slot)
        assert h.nvisible() == nvis and cc.counts(h) == (n, n - gone.size, gone.size)
        assert_same(*h.search(c.Q, K, 3), *c.search(oracle, c.Q, hmask & live, K, 3)[:2], f"{kind}: the handle's filter is what it was")
        # removed rows alone (no caller's filter): the bitmap is ANDed with liveness
        h.set_filter(None)
        _check(oracle, c, h, c.Q, call, (10,), 3, also=live, ctx=f"{kind}: live AND bitmap")
        # after compaction the bitmap is by the new positions
        h.set_filter(hmask)
        old = h.compact()
        assert np.array_equal(old, np.flatnonzero(live)) and h.ntotal == n - gone.size
        call2 = (rng.random(old.size) < 0.5).astype(np.uint8)
        for nprobe in (1, 3, 16):
            _check(oracle, c, h, c.Q, call2, (10, 100), nprobe, also=hmask[old], rows=old, ctx=f"{kind}: after compact, nprobe {nprobe}")
        with pytest.raises(ValueError):  # the old length is refused now: by the front end, and by the library
            h.search(c.Q, K, 3, bitmap=np.zeros(bc.nbytes(n), np.uint8))
        dist, lab, bits = np.full((1, K), -3.0, F), np.full((1, K), -9, np.int64), np.zeros(bc.nbytes(n), np.uint8)
        Q = np.ascontiguousarray(c.Q)
        rc = h._fn("search_bitmap_ctx")(h._h, 1, Q.ctypes.data, K, 3, bits.ctypes.data, n, 0, dist.ctypes.data, lab.ctypes.data, None)
        assert rc == INVALID and (dist == -3.0).all() and (lab == -9).all()
    finally:
        h.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_list_probed(oracle, kind):
    """pq and sq8: the flat code handle under set_filter with the same mask; rpq (distances per probed list: no flat counterpart):
    a second handle of its own under set_filter"""
    c = _first(oracle, kind)
    mask = fc.parity_masks()["10 % byte mask"]
    bits = bc.pack(mask)
    h = _handle(c)
    twin = c.k.flat(c.codes, c.par, c.dims) if c.k.flat_equal else _handle(c)
    try:
        twin.set_filter(mask)
        for k in (10, 100):
            want = twin.search(c.Q, k) if c.k.flat_equal else twin.search(c.Q, k, c.nlist)
            for nprobe in (16, 21):
                lab, dist = h.search(c.Q, k, nprobe, bitmap=bits)
                assert_same(lab, dist, *want, f"{kind} nprobe {nprobe} k {k}")
                assert h.last_search_stats()[1] == c.Q.shape[0] * np.count_nonzero(mask)
    finally:
        h.Close()
        twin.Close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2993, 2999])  # n % 8 == 1, 7
@pytest.mark.parametrize("kind", KINDS)
def test_device_bitmap_at_an_odd_address_with_ones_behind_it(oracle, kind, n):
    import torch
    c = _first(oracle, kind)
    rows = np.arange(n)
    assert n % 8 in (1, 7)
    mask = fc.parity_masks()["50 % byte mask"][:n].copy()
    mask[-1] = 0                                              # the last row is hidden, the bits behind it are ones
    bits = bc.pack(mask)
    bits[-1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
    nb = bc.nbytes(n)
    nq = c.Q.shape[0]
    h = _handle(c, rows=rows)
    try:
        buf = torch.full((nb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        buf[1:1 + nb] = torch.from_numpy(bits).cuda()
        assert (buf.data_ptr() + 1) % 2 == 1
        dQ = torch.from_numpy(np.array(c.Q, F)).cuda()
        dD = torch.empty((nq, K), dtype=torch.float32, device="cuda")
        dL = torch.empty((nq, K), dtype=torch.int64, device="cuda")
        for nprobe in (3, 16):
            torch.cuda.synchronize()
            h.search_device(nq, dQ.data_ptr(), K, nprobe, dD.data_ptr(), dL.data_ptr(), d_bitmap=buf.data_ptr() + 1, nbits=n)
            torch.cuda.synchronize()
            ol, od, scanned = c.search(oracle, c.Q, (mask != 0).astype(np.uint8), K, nprobe, rows=rows)
            assert_same(dL.cpu().numpy(), dD.cpu().numpy(), ol, od, f"{kind} n {n} nprobe {nprobe}")
            assert h.last_search_stats() == _stats(scanned, nq)
            assert n - 1 not in dL.cpu().numpy()
        # per query, strided, from an odd base too
        masks = bc.per_query_masks(nq, n)
        prow = bc.pack_rows(masks, stride=nb + 3, fill=0xFF)
        buf2 = torch.full((prow.size + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        buf2[3:3 + prow.size] = torch.from_numpy(prow.reshape(-1)).cuda()
        torch.cuda.synchronize()
        h.search_device(nq, dQ.data_ptr(), K, 3, dD.data_ptr(), dL.data_ptr(), d_bitmap=buf2.data_ptr() + 3, nbits=n, bitmap_stride=nb + 3)
        torch.cuda.synchronize()
        assert_same(dL.cpu().numpy(), dD.cpu().numpy(), *h.search(c.Q, K, 3, bitmap=prow, bitmap_stride=nb + 3), f"{kind}: strided device bitmap")
    finally:
        h.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_behind_a_live_handle(oracle, kind):
    c = _first(oracle, kind)
    n, nq = c.n, c.Q.shape[0]
    nb = bc.nbytes(n)
    Q = np.ascontiguousarray(c.Q)
    h = _handle(c)
    try:
        bits = np.full((nq, nb + 8), 0xFF, np.uint8)
        err = lambda: h._fn("last_error")(h._h).decode()
        host = h._fn("search_bitmap_ctx")

        def call(bitmap, nbits, stride, nprobe=3):
            dist = np.full((nq, K), -3.0, F)
            lab = np.full((nq, K), -9, np.int64)
            rc = host(h._h, nq, Q.ctypes.data, K, nprobe, bitmap, nbits, stride, dist.ctypes.data, lab.ctypes.data, None)
            return rc, dist, lab

        for nbits, stride, words in ((n + 1, 0, (str(n + 1), str(n))), (n - 1, 0, (str(n - 1), str(n))), (-1, 0, ("-1", str(n))),
                                     (n, -1, ("-1",)), (n, nb - 1, (str(nb - 1), str(nb))), (n, 1, ("1", str(nb)))):
            rc, dist, lab = call(bits.ctypes.data, nbits, stride)
            assert rc == INVALID, (nbits, stride)
            assert (dist == -3.0).all() and (lab == -9).all(), (nbits, stride)
            assert "bitmap" in err() and all(w in err() for w in words), (err(), words)
        assert h.nvisible() == n
        # a NULL bitmap is the plain search, whatever nbits and the stride say
        want = h.search(c.Q, K, 3)
        rc, dist, lab = call(None, -5, -7)
        assert rc == OK
        assert_same(lab, dist, *want, "NULL bitmap")
        # a stride of exactly ceil(n / 8) and a larger one are taken
        assert call(bits.ctypes.data, n, nb)[0] == OK and call(bits.ctypes.data, n, nb + 8)[0] == OK
        # the plain entry points' checks come first, with their texts
        rc, dist, lab = call(bits.ctypes.data, n + 1, 0, nprobe=0)
        assert rc == INVALID and "nprobe" in err() and (dist == -3.0).all()
        # a correct search right after still answers
        _check(oracle, c, h, c.Q, fc.parity_masks()["10 % byte mask"], (10,), 3, ctx=f"{kind}: after the refusals")
    finally:
        h.Close()
    # an empty handle answers all padding with or without a bitmap, and its first add is found
    e = _handle(c, rows=np.arange(0))
    try:
        lab, dist = e.search(c.Q, K, 3, bitmap=np.zeros(0, np.uint8))
        assert (lab == -1).all() and (dist == FLT_MAX).all() and e.last_search_stats() == (nq, 0, 0, 0)
    finally:
        e.Close()


# 11 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_threads_two_bitmaps_one_handle_and_a_fired_context(oracle, kind):
    from longbow_amd import gpu
    c = _first(oracle, kind)
    masks = fc.parity_masks()
    h = _handle(c)
    try:
        jobs = []
        for name in ("10 % byte mask", "50 % byte mask"):
            bits = bc.pack(masks[name])
            jobs.append((bits, kc.search_bitmap(oracle, c, c.Q, bits, K, 3)[:2]))
        wrong, errors = [], []

        def work(i):
            bits, (ol, od) = jobs[i]
            try:
                for it in range(20):
                    lab, dist = h.search(c.Q, K, 3, bitmap=bits)
                    if not (np.array_equal(lab, ol) and np.array_equal(dist, od)):
                        wrong.append((i, it))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors and not wrong, (errors, wrong[:5])
        assert h.nvisible() == c.n
        # a fired context cancels, writes nothing, and the next search is right
        ctx = gpu.Cancel()
        ctx.fire()
        Q = np.ascontiguousarray(c.Q)
        dist = np.full((Q.shape[0], K), -3.0, F)
        lab = np.full((Q.shape[0], K), -9, np.int64)
        bits = jobs[0][0]
        rc = h._fn("search_bitmap_ctx")(h._h, Q.shape[0], Q.ctypes.data, K, 3, bits.ctypes.data, c.n, 0, dist.ctypes.data, lab.ctypes.data, ctx._h)
        assert rc == CANCELLED and (dist == -3.0).all() and (lab == -9).all()
        _check(oracle, c, h, c.Q, masks["10 % byte mask"], (10,), 3, ctx=f"{kind}: after a cancelled call")
    finally:
        h.Close()


# 12 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pq", "sq8"])
def test_search_refine_under_a_bitmap(oracle, kind):
    c = _first(oracle, kind)
    mask = (fc.parity_masks()["10 % byte mask"] != 0).astype(np.uint8)
    bits = bc.pack(mask)
    h = _handle(c)
    idx = new_index(c.dims)
    try:
        idx.Add(None, c.X)
        short, _, _ = c.search(oracle, c.Q, mask, 64, 2)  # the oracle's shortlist under the mask
        for order in (0, 1):
            lab, dist = h.search_refine(idx, c.Q, 5, 64, 2, order=order, bitmap=bits)
            assert_same(lab, dist, *fo.refine(oracle, 0, c.Q, c.X, short, 5, order), f"{kind} order {order}")
            assert mask[lab[lab >= 0]].all()
        # a bitmap per query goes the same way
        masks = bc.per_query_masks(c.Q.shape[0], c.n)
        pb = bc.pack_rows(masks)
        lab, _ = h.search_refine(idx, c.Q, 5, 64, 2, bitmap=pb, bitmap_stride=bc.nbytes(c.n))
        for q in range(c.Q.shape[0]):
            assert masks[q][lab[q][lab[q] >= 0]].all()
        assert (lab[0] == -1).all()
    finally:
        idx.Close()
        h.Close()


# 13 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlist,nrows,nq", [(300, 3000, 33), (300, 200, 33), (LB_MAX_K + 52, 3000, 4)])
@pytest.mark.parametrize("kind", KINDS)
def test_many_lists_all_probed(oracle, kind, nlist, nrows, nq):
    """300 lists: under one compaction per call the walk of the lists' starts takes more than one round of a wave's 64 lanes, and
    with 200 rows there are more lists than rows, most of them empty.  2,100 lists all probed is more probes than the coarse search
    returns (LB_MAX_K): the probes are every list in order, without it.  Every call here is on the shared side of the rule."""
    p = _first(oracle, kind)
    C_ = np.random.default_rng(55 + nlist).standard_normal((nlist, p.dims)).astype(F)
    c = cc.Case(oracle, kind, p.X[:nrows], p.Q[:nq], C_, p.par)
    mask = (fc.parity_masks()["50 % byte mask"][:nrows] != 0).astype(np.uint8)
    h = _handle(c)
    try:
        assert _shared(h, nq, nlist)
        scanned = _check(oracle, c, h, c.Q, mask, (10, 100), nlist, ctx=f"{kind}: {nlist} lists over {nrows} rows, all probed")
        assert (scanned == np.count_nonzero(mask)).all()
        if nlist <= LB_MAX_K:
            _check(oracle, c, h, c.Q, mask, (10,), 70, ctx=f"{kind}: {nlist} lists over {nrows} rows, 70 probed")
            _check(oracle, c, h, c.Q[:1], mask, (10,), 2, ctx=f"{kind}: {nlist} lists over {nrows} rows, one query, 2 probed")
    finally:
        h.Close()


# the IVF-Flat handle goes through the same loop: its batched calls under one bitmap now compact every list once
@pytest.mark.parametrize("rows", ["float32", "float16", "int8"])
def test_ivf_flat_33_equal_bitmaps_against_one(rows):
    from longbow_amd import ivf
    from longbow_amd.gpu import DataType
    gpu_or_skip()
    X, Q, C_ = io.parity_case()
    if rows == "int8":
        X, Q, C_ = o8.to_i8(X, 30), o8.to_i8(Q, 30), (C_ * F(30)).astype(F)
        h = ivf.IVFFlatInt8(C_)
    elif rows == "float16":
        X = X.astype(np.float16)
        h = ivf.IVFFlat(C_, 0, 0, dtype=DataType.Float16)
    else:
        h = ivf.IVFFlat(C_, 0, 0)
    try:
        h.add(X)
        n, nq = X.shape[0], Q.shape[0]
        mask = (fc.parity_masks()["50 % byte mask"] != 0).astype(np.uint8)
        strided = bc.pack_rows(np.broadcast_to(mask, (nq, n)))
        for nprobe in (1, 3, 16):
            assert kc.shared_form(h.list_sizes(), nq, nprobe, 0) and not kc.shared_form(h.list_sizes(), nq, nprobe, bc.nbytes(n))
            a = h.search(Q, K, nprobe, bitmap=strided, bitmap_stride=bc.nbytes(n))
            sa = h.last_search_stats()
            b = h.search(Q, K, nprobe, bitmap=strided[0])
            assert_same(*a, *b, f"{rows} nprobe {nprobe}")
            assert sa == h.last_search_stats()
            h.set_filter(mask)
            assert_same(*b, *h.search(Q, K, nprobe), f"{rows} nprobe {nprobe}: set_filter")
            assert sa == h.last_search_stats()
            h.set_filter(None)
    finally:
        h.Close()
