"""A row bitmap given with the search call on the IVF-Flat handle (lb_gpu_ivf_search_bitmap_ctx / _bitmap_device_ctx and the _i8
forms) on the GPU.  The expected result everywhere is tests/ivf_filter_cases.py's search_filtered under the unpacked bits
(tests/ivf_bitmap_cases.py, pinned on the CPU by tests/test_ivf_bitmap_semantics.py), ANDed with the handle's own mask and with
liveness where a test sets them; labels and distances are compared for equality and lb_gpu_ivf_last_search_stats shows that the
search walked the passing rows alone.  The shapes are the smallest at which the compaction of the probed lists, and the search
sized by the handle's unfiltered list sizes, can go wrong: list lengths and kept counts around the compaction's 2048-position step
and the scan's 128-row tile, lists emptied by the bitmap, the selection's 16,384 LDS keys under an unfiltered bound beyond them,
more lists than rows, bitmaps at odd addresses with ones behind their last bit."""
import threading

import numpy as np
import pytest

from tests import ivf_bitmap_cases as bc
from tests import ivf_filter_cases as fc
from tests import ivf_i8_oracle as o8
from tests import ivf_oracle as io
from tests.gpu_util import assert_same, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
OK, INVALID, CANCELLED = 0, 1, 8
K = fc.K


def _handle(X, C_, metric=0, order=0, ids=None, dtype=None):
    from longbow_amd import ivf
    gpu_or_skip()
    h = ivf.IVFFlat(C_, metric, order) if dtype is None else ivf.IVFFlat(C_, metric, order, dtype=dtype)
    if X.shape[0]:
        h.add(X, ids)
    return h


def _stats(scanned, nq):
    return (nq, int(scanned.sum()), int(scanned.max()), int((scanned <= fc.LDS_KEYS).sum()))


def _check(oracle, h, metric, order, Q, X, C_, lists, mask, k, nprobe, also=None, ids=None, ctx=""):
    """labels, distances and all four counters of a search under the bitmap of `mask` against the helper -> rows scanned"""
    bits = bc.pack(mask)
    ol, od, scanned = bc.search_bitmap(oracle, metric, order, Q, X, C_, lists, bits, k, nprobe, ids=ids, also=also)
    lab, dist = h.search(Q, k, nprobe, bitmap=bits)
    assert_same(lab, dist, ol, od, ctx)
    assert h.last_search_stats() == _stats(scanned, Q.shape[0]), (h.last_search_stats(), scanned.sum(), scanned.max(), ctx)
    return scanned


@pytest.fixture(scope="module")
def parity(oracle):
    X, Q, C_ = io.parity_case()
    return X, Q, C_, io.assign(oracle, 0, 0, X, C_)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,order", [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)])
def test_parity_under_every_mask_as_a_bitmap(oracle, metric, order):
    X, Q, C_ = io.parity_case()
    lists = io.assign(oracle, metric, order, X, C_)
    h = _handle(X, C_, metric, order)
    plain = {nprobe: (h.search(Q, K, nprobe), h.last_search_stats()) for nprobe in (1, 3, 16)}
    masks = fc.parity_masks()
    names = list(masks) if (metric, order) == (0, 0) else ["10 % byte mask", "50 % byte mask"]
    for name in names:
        for nprobe in (1, 3, 16):
            _check(oracle, h, metric, order, Q, X, C_, lists, masks[name], K, nprobe, ctx=f"{name}, metric {metric} order {order} nprobe {nprobe}")
            # the handle is what it was: no filter on it, and the plain search answers as before
            assert h.nvisible() == h.ntotal == X.shape[0]
            assert_same(*h.search(Q, K, nprobe), *plain[nprobe][0], f"plain search after {name}")
            assert h.last_search_stats() == plain[nprobe][1]
    h.Close()


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["float32", "float16", "int8"])
def test_equal_to_the_same_handle_under_set_filter(kind):
    from longbow_amd import ivf
    from longbow_amd.gpu import DataType
    gpu_or_skip()
    X, Q, C_ = io.parity_case()
    if kind == "int8":
        X, Q, C_ = o8.to_i8(X, 30), o8.to_i8(Q, 30), (C_ * F(30)).astype(F)
        h = ivf.IVFFlatInt8(C_)
        h.add(X)
    elif kind == "float16":
        h = _handle(X.astype(np.float16), C_, dtype=DataType.Float16)
    else:
        h = _handle(X, C_)
    masks = fc.parity_masks()
    for name in ("10 % byte mask", "50 % byte mask", "row 0", "all-zero", "all-one"):
        bits = bc.pack(masks[name])
        got = {nprobe: (h.search(Q, K, nprobe, bitmap=bits), h.last_search_stats()) for nprobe in (1, 3, 16)}
        assert h.nvisible() == X.shape[0]
        h.set_filter(masks[name])
        for nprobe, ((lab, dist), st) in got.items():
            assert_same(lab, dist, *h.search(Q, K, nprobe), f"{kind} {name} nprobe {nprobe}")
            assert st == h.last_search_stats(), (kind, name, nprobe)
        h.set_filter(None)
    h.Close()


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("choice", ["first rows", "random rows"])
@pytest.mark.parametrize("case", ["compaction step", "scan tile"])
def test_kept_counts_at_the_edges_of_the_step_and_the_tile(oracle, case, choice):
    counts, keep = (bc.STEP_COUNTS, bc.STEP_KEEP) if case == "compaction step" else (fc.EDGE_COUNTS, fc.EDGE_KEEP)
    X, Q, C_, owner = io.edge_case(counts)
    mask = fc.keep_per_list(owner, keep, None if choice == "first rows" else np.random.default_rng(6))
    h = _handle(X, C_)
    assert h.list_sizes().tolist() == list(counts)
    for nprobe in (1, 2):
        for k in (10, 200):
            scanned = _check(oracle, h, 0, 0, Q, X, C_, owner, mask, k, nprobe, ctx=f"{case}, {choice} nprobe {nprobe} k {k}")
            if nprobe == 1:
                assert scanned.tolist() == list(keep)
    lab, dist = h.search(Q, 10, 1, bitmap=bc.pack(mask))
    assert (lab[0] == -1).all() and (dist[0] == io.FLT_MAX).all()  # a probed list with no set bit: all padding
    assert lab[1, 0] == np.flatnonzero((owner == 1) & (mask != 0))[0] and (lab[1, 1:] == -1).all() and (dist[1, 1:] == io.FLT_MAX).all()
    assert h.list_sizes().tolist() == list(counts) and h.nvisible() == X.shape[0]
    h.Close()


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_the_selection_follows_the_kept_count_not_the_bound(oracle):
    """list 0 holds about 37,000 rows, so pmax, which stays the unfiltered bound, is beyond every selection from LDS; with exactly
    16,384 of its bits set the three queries that probe it are selected from LDS, with one more they are not"""
    X, Q, C_ = io.skew_case()
    lists = io.assign(oracle, 0, 0, X, C_)
    assert np.bincount(lists)[0] > 2 * fc.LDS_KEYS
    h = _handle(X, C_)
    for keep0, from_lds in ((fc.LDS_KEYS, 5), (fc.LDS_KEYS + 1, 2)):
        mask = fc.skew_mask(lists, keep0)
        for k in (10, 100):
            _check(oracle, h, 0, 0, Q, X, C_, lists, mask, k, 1, ctx=f"{keep0} bits set in list 0, k {k}")
            assert h.last_search_stats()[3] == from_lds
    h.Close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_a_bitmap_per_query(oracle, parity):
    X, Q, C_, lists = parity
    n, nq = X.shape[0], Q.shape[0]
    masks = bc.per_query_masks(nq, n)
    h = _handle(X, C_)
    for stride, fill in ((bc.nbytes(n), 0), (bc.nbytes(n) + 5, 0xFF)):
        bits = bc.pack_rows(masks, stride=stride, fill=fill)
        for nprobe in (1, 3, 16):
            lab, dist = h.search(Q, K, nprobe, bitmap=bits, bitmap_stride=stride)
            st = h.last_search_stats()
            scanned = np.empty(nq, np.int64)
            for q in range(nq):  # each row is the single-bitmap search of that query: on the GPU, and in the oracle
                l1, d1 = h.search(Q[q:q + 1], K, nprobe, bitmap=bits[q, :bc.nbytes(n)])
                assert_same(lab[q:q + 1], dist[q:q + 1], l1, d1, f"stride {stride} nprobe {nprobe} query {q}")
                scanned[q] = h.last_search_stats()[1]
            assert st == _stats(scanned, nq)
            assert (lab[0] == -1).all() and scanned[0] == 0                   # the all-zero bitmap
            if nprobe == 3:
                ol, od, osc = bc.search_strided(oracle, 0, 0, Q, X, C_, lists, bits, K, nprobe)
                assert_same(lab, dist, ol, od, f"stride {stride} against the oracle")
                assert np.array_equal(scanned, osc)
    from longbow_amd import ivf
    pb, ps = ivf.pack_bitmap(masks)
    assert_same(*h.search(Q, K, 3, bitmap=pb, bitmap_stride=ps), *h.search(Q, K, 3, bitmap=bc.pack_rows(masks), bitmap_stride=bc.nbytes(n)), "pack_bitmap")
    h.Close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_and_with_the_handle_filter_and_with_removed_rows(oracle, parity):
    X, Q, C_, lists = parity
    n = X.shape[0]
    rng = np.random.default_rng(21)
    masks = fc.parity_masks()
    hmask = (masks["50 % byte mask"] != 0).astype(np.uint8)
    gone = np.sort(rng.permutation(n)[:400])
    live = np.ones(n, np.uint8)
    live[gone] = 0
    call = (rng.random(n) < 0.5).astype(np.uint8)
    h = _handle(X, C_)
    h.set_filter(hmask)
    assert h.remove_rows(gone) == 400
    nvis = h.nvisible()
    assert nvis == np.count_nonzero(hmask & live)
    for nprobe in (1, 3, 16):
        scanned = _check(oracle, h, 0, 0, Q, X, C_, lists, call, K, nprobe, also=hmask & live, ctx=f"filter AND live AND bitmap, nprobe {nprobe}")
        assert scanned.sum() < fc.search_filtered(oracle, 0, 0, Q, X, C_, lists, hmask & live, K, nprobe)[2].sum()
    assert h.nvisible() == nvis
    # removed rows alone (no caller's filter): the bitmap is ANDed with liveness
    h.set_filter(None)
    _check(oracle, h, 0, 0, Q, X, C_, lists, call, K, 3, also=live, ctx="live AND bitmap")
    # after compaction the bitmap is by the new positions
    h.set_filter(hmask)
    old = h.compact()
    assert np.array_equal(old, np.flatnonzero(live)) and h.ntotal == n - 400
    call2 = (rng.random(n - 400) < 0.5).astype(np.uint8)
    _check(oracle, h, 0, 0, Q, X[old], C_, lists[old], call2, K, 3, also=hmask[old], ctx="after compact")
    with pytest.raises(ValueError):  # the old length is refused now: by the front end, and by the library
        h.search(Q, K, 3, bitmap=np.zeros(bc.nbytes(n), np.uint8))
    dist, lab, bits = np.full((1, K), -3.0, F), np.full((1, K), -9, np.int64), np.zeros(bc.nbytes(n), np.uint8)
    rc = h._lib.lb_gpu_ivf_search_bitmap_ctx(h._h, 1, Q.ctypes.data, K, 3, bits.ctypes.data, n, 0, dist.ctypes.data, lab.ctypes.data, None)
    assert rc == INVALID and (dist == -3.0).all() and (lab == -9).all()
    h.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_every_list_probed_equals_the_filtered_flat_index(metric):
    X, Q, C_ = io.parity_case()
    mask = fc.parity_masks()["10 % byte mask"]
    bits = bc.pack(mask)
    for order in (0, 1):
        h = _handle(X, C_, metric, order)
        flat = new_index(X.shape[1], metric, order)
        flat.Add(None, X)
        flat.set_filter(mask)
        fl, fd = flat.SearchBatch(Q, K)
        for nprobe in (16, 21):
            lab, dist = h.search(Q, K, nprobe, bitmap=bits)
            assert_same(lab, dist, fl, fd, f"metric {metric} order {order} nprobe {nprobe}")
            assert h.last_search_stats()[1] == Q.shape[0] * np.count_nonzero(mask)
        flat.Close()
        h.Close()


def test_more_lists_than_rows_and_an_empty_handle(oracle):
    X, Q, _ = io.parity_case(n=10, nq=9)
    C_ = np.random.default_rng(55).standard_normal((64, X.shape[1])).astype(F)
    lists = io.assign(oracle, 0, 0, X, C_)
    h = _handle(X, C_)
    for mask in (np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1], np.uint8), np.zeros(10, np.uint8), np.ones(10, np.uint8)):
        for nprobe in (1, 7, 64, 100):
            _check(oracle, h, 0, 0, Q, X, C_, lists, mask, K, nprobe, ctx=f"64 lists, 10 rows, nprobe {nprobe}")
    h.Close()
    h = _handle(X[:0], C_)
    lab, dist = h.search(Q, K, 3, bitmap=np.zeros(0, np.uint8))
    assert (lab == -1).all() and (dist == io.FLT_MAX).all() and h.last_search_stats() == (Q.shape[0], 0, 0, 0)
    h.add(X)
    _check(oracle, h, 0, 0, Q, X, C_, lists, np.ones(10, np.uint8), K, 64, ctx="after the first add")
    h.Close()


# 8 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2993, 2999])  # n % 8 == 1, 7
def test_device_bitmap_at_an_odd_address_with_ones_behind_it(oracle, parity, n):
    import torch
    X, Q, C_, lists = parity
    X, lists = X[:n], lists[:n]
    assert n % 8 in (1, 7)
    mask = fc.parity_masks()["50 % byte mask"][:n]
    mask[-1] = 0                                              # the last row is hidden, the bits behind it are ones
    bits = bc.pack(mask)
    bits[-1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
    nb = bc.nbytes(n)
    h = _handle(X, C_)
    buf = torch.full((nb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[1:1 + nb] = torch.from_numpy(bits).cuda()
    assert (buf.data_ptr() + 1) % 2 == 1
    dQ = torch.from_numpy(Q).cuda()
    for nprobe in (3, 16):
        dD = torch.empty((Q.shape[0], K), dtype=torch.float32, device="cuda")
        dL = torch.empty((Q.shape[0], K), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        h.search_device(Q.shape[0], dQ.data_ptr(), K, nprobe, dD.data_ptr(), dL.data_ptr(), d_bitmap=buf.data_ptr() + 1, nbits=n)
        ol, od, scanned = fc.search_filtered(oracle, 0, 0, Q, X, C_, lists, mask, K, nprobe)
        assert_same(dL.cpu().numpy(), dD.cpu().numpy(), ol, od, f"n {n} nprobe {nprobe}")
        assert h.last_search_stats() == _stats(scanned, Q.shape[0])
        assert n - 1 not in dL.cpu().numpy()
    # per query, strided, from an odd base too
    masks = bc.per_query_masks(Q.shape[0], n)
    rows = bc.pack_rows(masks, stride=nb + 3, fill=0xFF)
    buf2 = torch.full((rows.size + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    buf2[3:3 + rows.size] = torch.from_numpy(rows.reshape(-1)).cuda()
    torch.cuda.synchronize()
    h.search_device(Q.shape[0], dQ.data_ptr(), K, 3, dD.data_ptr(), dL.data_ptr(), d_bitmap=buf2.data_ptr() + 3, nbits=n, bitmap_stride=nb + 3)
    assert_same(dL.cpu().numpy(), dD.cpu().numpy(), *h.search(Q, K, 3, bitmap=rows, bitmap_stride=nb + 3), "strided device bitmap")
    h.Close()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_behind_a_live_handle(parity):
    from longbow_amd import ivf
    X, Q, C_, lists = parity
    n, nq = X.shape[0], Q.shape[0]
    nb = bc.nbytes(n)
    h = _handle(X, C_)
    lib = h._lib
    bits = np.full((nq, nb + 8), 0xFF, np.uint8)
    err = lambda: lib.lb_gpu_ivf_last_error(h._h).decode()

    def call(fn, q, bitmap, nbits, stride):
        dist = np.full((nq, K), -3.0, F)
        lab = np.full((nq, K), -9, np.int64)
        rc = fn(h._h, nq, q.ctypes.data, K, 3, bitmap, nbits, stride, dist.ctypes.data, lab.ctypes.data, None)
        return rc, dist, lab

    host = lib.lb_gpu_ivf_search_bitmap_ctx
    for nbits, stride, words in ((n + 1, 0, (str(n + 1), str(n))), (n - 1, 0, (str(n - 1), str(n))), (-1, 0, ("-1", str(n))),
                                 (n, -1, ("-1",)), (n, nb - 1, (str(nb - 1), str(nb))), (n, 1, ("1", str(nb)))):
        rc, dist, lab = call(host, Q, bits.ctypes.data, nbits, stride)
        assert rc == INVALID, (nbits, stride)
        assert (dist == -3.0).all() and (lab == -9).all(), (nbits, stride)
        assert "bitmap" in err() and all(w in err() for w in words), (err(), words)
    assert h.nvisible() == n
    # a NULL bitmap is the plain search, whatever nbits and the stride say
    want = h.search(Q, K, 3)
    rc, dist, lab = call(host, Q, None, -5, -7)
    assert rc == OK
    assert_same(lab, dist, *want, "NULL bitmap")
    # a stride of exactly ceil(n / 8) and a larger one are taken
    assert call(host, Q, bits.ctypes.data, n, nb)[0] == OK and call(host, Q, bits.ctypes.data, n, nb + 8)[0] == OK
    # the plain entry points' checks come first, with their texts
    rc, dist, lab = call(host, Q, bits.ctypes.data, n + 1, 0)
    dist2 = np.full((nq, K), -3.0, F)
    assert host(h._h, nq, Q.ctypes.data, K, 0, bits.ctypes.data, n + 1, 0, dist2.ctypes.data, lab.ctypes.data, None) == INVALID and "nprobe" in err()
    # the other element type's forms
    Q8 = o8.to_i8(Q, 30)
    rc, dist, lab = call(lib.lb_gpu_ivf_search_i8_bitmap_ctx, Q8, bits.ctypes.data, n, 0)
    assert rc == INVALID and "float32" in err() and (dist == -3.0).all() and (lab == -9).all()
    h8 = ivf.IVFFlatInt8((C_ * F(30)).astype(F))
    h8.add(o8.to_i8(X, 30))
    dist = np.full((nq, K), -3.0, F)
    lab = np.full((nq, K), -9, np.int64)
    assert host(h8._h, nq, Q.ctypes.data, K, 3, bits.ctypes.data, n, 0, dist.ctypes.data, lab.ctypes.data, None) == INVALID
    assert "int8" in lib.lb_gpu_ivf_last_error(h8._h).decode() and (dist == -3.0).all() and (lab == -9).all()
    assert lib.lb_gpu_ivf_search_i8_bitmap_ctx(h8._h, nq, Q8.ctypes.data, K, 3, bits.ctypes.data, n + 1, 0, dist.ctypes.data, lab.ctypes.data, None) == INVALID
    assert "bitmap" in lib.lb_gpu_ivf_last_error(h8._h).decode() and (dist == -3.0).all() and (lab == -9).all()
    h8.Close()
    h.Close()


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_two_threads_two_bitmaps_one_handle(oracle, parity):
    X, Q, C_, lists = parity
    masks = fc.parity_masks()
    h = _handle(X, C_)
    jobs = []
    for name in ("10 % byte mask", "50 % byte mask"):
        bits = bc.pack(masks[name])
        jobs.append((bits, bc.search_bitmap(oracle, 0, 0, Q, X, C_, lists, bits, K, 3)[:2]))
    wrong, errors = [], []

    def work(i):
        bits, (ol, od) = jobs[i]
        try:
            for it in range(32):
                lab, dist = h.search(Q, K, 3, bitmap=bits)
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
    assert h.nvisible() == X.shape[0]
    h.Close()


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_a_fired_context_cancels_and_the_next_search_is_right(oracle, parity):
    from longbow_amd import gpu
    X, Q, C_, lists = parity
    mask = fc.parity_masks()["10 % byte mask"]
    bits = bc.pack(mask)
    h = _handle(X, C_)
    lib = h._lib
    c = gpu.Cancel()
    c.fire()
    dist = np.full((Q.shape[0], K), -3.0, F)
    lab = np.full((Q.shape[0], K), -9, np.int64)
    rc = lib.lb_gpu_ivf_search_bitmap_ctx(h._h, Q.shape[0], Q.ctypes.data, K, 3, bits.ctypes.data, X.shape[0], 0, dist.ctypes.data, lab.ctypes.data, c._h)
    assert rc == CANCELLED and (dist == -3.0).all() and (lab == -9).all()
    _check(oracle, h, 0, 0, Q, X, C_, lists, mask, K, 3, ctx="after a cancelled call")
    h.Close()


# the reference's SearchVectorsWithBitmap on the ivf_flat index type
def test_python_mirror(oracle, parity):
    from longbow_amd import ivf
    X, Q, C_, lists = parity
    n = X.shape[0]
    ids = np.arange(n, dtype=np.int64) + (1 << 33)
    idx = ivf.IVFFlatIndex(X.shape[1], ivf.IVFFlatConfig(NClusters=16, NProbe=3), centroids=C_)
    idx.AddBatch(ids, X)
    idx.Build()
    mask = fc.parity_masks()["10 % byte mask"]
    bits, stride = ivf.pack_bitmap(mask)
    assert stride == 0
    ol, od, _ = fc.search_filtered(oracle, 0, 0, Q, X, C_, lists, mask, K, 3, ids=ids)
    assert_same(*idx.SearchBatch(Q, K, bitmap=bits), ol, od, "SearchBatch under a bitmap")
    l1, d1 = idx.Search(Q[4], K, bitmap=bits)
    assert np.array_equal(l1, ol[4]) and np.array_equal(d1, od[4])
    assert idx.nvisible() == n
    with pytest.raises(ValueError):
        idx.SearchBatch(Q, K, bitmap=bits[:-1])
    idx.Close()
