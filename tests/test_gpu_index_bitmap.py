"""A row bitmap given with the search call on the flat index (include/longbow_gpu.h, lb_gpu_index_*: "call bitmap";
kernels_index_call.hip, build_call_view in index_search.hip) against the oracle under the unpacked bits, and against the same index
under set_filter.  Shapes and the expected result come from tests/index_bitmap_cases.py; tests/test_index_bitmap_semantics.py pins
them on the CPU.  Every comparison is exact: labels and distances bit for bit."""
import threading

import numpy as np
import pytest

from tests import index_bitmap_cases as ic
from tests import ivf_bitmap_cases as bc
from tests import row_view_cases as rc
from tests.gpu_util import assert_same, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
L2, COS, DOT = 0, 1, 2
FLT_MAX = np.finfo(F).max
OK, INVALID, CANCELLED = 0, 1, 8


# ---- shared corpora (computed once, never written to) ---------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """2049 x 8: searched with k = 2048, the labels that are not -1 are exactly the visible rows"""
    rng = np.random.default_rng(100)
    X, q = rng.random((2049, 8), dtype=F), rng.random((1, 8), dtype=F)
    X.setflags(write=False)
    return X, q


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(101)
    n, d = 20000, 32
    X, Q = rng.random((n, d), dtype=F), rng.random((385, d), dtype=F)
    Q[0] = X[n // 3]  # the row rc.structured_masks' "all but one" hides is query 0's nearest neighbour
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


@pytest.fixture(scope="module")
def filled(corpus):
    """one f32 L2 index over the corpus, never filtered, shared by the tests that leave a handle as they found it"""
    gpu_or_skip()
    X, _ = corpus
    idx = new_index(X.shape[1], L2)
    idx.Add(None, X)
    yield idx
    idx.Close()


def dev_search(idx, Q, k, bits, n, offset=1, stream=None):
    """search_device with the bitmap in device memory `offset` bytes into a buffer of 0xFF, so that the byte in front of it and
    the bytes behind it are ones -> (labels, dist) as numpy"""
    import torch
    tq = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16, np.dtype(np.int8): torch.int8}[Q.dtype]
    nb = bc.nbytes(n)
    buf = torch.full((offset + nb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    if nb:
        buf[offset:offset + nb] = torch.from_numpy(np.ascontiguousarray(bits, np.uint8)).cuda()
    dQ = torch.from_numpy(np.array(Q)).to(device="cuda", dtype=tq)  # (a copy: the shared corpora are read-only)
    dD = torch.empty((Q.shape[0], k), dtype=torch.float32, device="cuda")
    dL = torch.empty((Q.shape[0], k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    idx.search_device(Q.shape[0], dQ.data_ptr(), k, dD.data_ptr(), dL.data_ptr(), stream=stream, d_bitmap=buf.data_ptr() + offset, nbits=n)
    return dL.cpu().numpy(), dD.cpu().numpy()


# 1 ---- parity against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 200])
@pytest.mark.parametrize("metric", [L2, COS, DOT])
def test_parity_against_the_oracle(oracle, corpus, metric, k):
    gpu_or_skip()
    X, Q = corpus
    n = X.shape[0]
    idx = new_index(X.shape[1], metric)
    try:
        idx.Add(None, X)
        for name, mask in rc.structured_masks(n, k, np.random.default_rng(k)).items():
            bits = bc.pack(mask)
            ol, od = ic.search_bitmap(oracle, metric, Q, X, k, bits)
            for nq in (1, 4, 5, 64, 385):
                lab, dist = idx.SearchBatch(Q[:nq], k, bitmap=bits)
                assert_same(lab, dist, ol[:nq], od[:nq], f"metric {metric} k {k} mask '{name}' nq {nq}")
            nv = int(mask.sum())
            if nv < k:
                assert np.all(ol[:, nv:] == -1) and np.all(od[:, nv:] == FLT_MAX)
        assert idx.nvisible() == n
    finally:
        idx.Close()


def test_parity_on_the_fp16_image_routes_under_a_row_list(oracle):
    """20,000 x 256, k = 100, 64 queries, 90 % of the rows visible: a row list of 18,000 rows, long enough for a sampled
    threshold and wide enough (dimension >= 256) for the routes over the index's fp16 image"""
    gpu_or_skip()
    rng = np.random.default_rng(102)
    n, d, k = 20000, 256, 100
    X, Q = rng.random((n, d), dtype=F), rng.random((64, d), dtype=F)
    mask = rc.exact_count_mask(rng, n, 18000)
    assert rc.takes_row_list(18000, n)
    idx = new_index(d, L2)
    try:
        idx.Add(None, X)
        lab, dist = idx.SearchBatch(Q, k, bitmap=bc.pack(mask))
        assert_same(lab, dist, *ic.search_bitmap(oracle, L2, Q, X, k, bc.pack(mask)), "20000 x 256")
        kind = idx.last_route[0]
        assert kind != 0, "the batch took the exact scan"
        # the same batch on the same index under set_filter answers the same
        idx.set_filter(mask)
        lab2, dist2 = idx.SearchBatch(Q, k)
        assert_same(lab, dist, lab2, dist2, "set_filter")
    finally:
        idx.Close()


# 2 ---- equal to the same index under set_filter ---------------------------------------------------------------------
def _typed(dtype, X, Q):
    from longbow_amd import gpu
    if dtype == "f16":
        return gpu.DataType.Float16, X.astype(np.float16), Q.astype(np.float16)
    if dtype == "i8":
        to8 = lambda a: np.clip(np.rint(a * 200 - 100), -127, 127).astype(np.int8)
        return gpu.DataType.Int8, to8(X), to8(Q)
    return gpu.DataType.Float32, X, Q


@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_equal_to_the_same_index_under_set_filter(corpus, dtype):
    gpu_or_skip()
    from longbow_amd import gpu
    X, Q = corpus
    n, k = X.shape[0], 10
    dt, Xt, Qt = _typed(dtype, X, Q[:64])
    rng = np.random.default_rng(3)
    masks = {"10 %": rc.byte_mask(rng, n, 0.1), "50 %": rc.byte_mask(rng, n, 0.5), "row 0": (np.arange(n) == 0).astype(np.uint8),
             "all zero": np.zeros(n, np.uint8), "all one": np.ones(n, np.uint8)}
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=X.shape[1], Metric=L2, DataType=dt))
    try:
        idx.Add(None, Xt)
        for name, mask in masks.items():
            bits = gpu.pack_bitmap(mask)[0]
            got = {nq: idx.SearchBatch(Qt[:nq], k, bitmap=bits) for nq in (1, 64)}
            dev = dev_search(idx, Qt, k, bits, n)
            assert idx.nvisible() == n
            idx.set_filter(mask)
            for nq in (1, 64):
                assert_same(*got[nq], *idx.SearchBatch(Qt[:nq], k), f"{dtype} mask '{name}' nq {nq}")
            assert_same(*dev, *idx.SearchBatch(Qt, k), f"{dtype} mask '{name}' device form")
            idx.set_filter(None)
            if name == "all zero":
                assert np.all(got[64][0] == -1) and np.all(got[64][1] == FLT_MAX)
    finally:
        idx.Close()


# 3 ---- the view rule's edge -----------------------------------------------------------------------------------------
def test_view_rule_edge(oracle, corpus, filled):
    X, Q = corpus
    n, k = X.shape[0], 10
    counts = ic.view_edge_counts(n)
    assert {lst for _, lst in counts} == {True, False}          # the list form and the per-row mask form both run
    for c, lst in counts:
        mask = rc.exact_count_mask(np.random.default_rng(c), n, c)
        assert int(mask.sum()) == c and rc.takes_row_list(c, n) == lst
        bits = bc.pack(mask)
        ol, od = ic.search_bitmap(oracle, L2, Q[:64], X, k, bits)
        for nq in (1, 64):
            assert_same(*filled.SearchBatch(Q[:nq], k, bitmap=bits), ol[:nq], od[:nq], f"{c} visible (list: {lst}) nq {nq}")
    assert filled.nvisible() == n


# 4 ---- the new kernel's edges ---------------------------------------------------------------------------------------
def _check_small(idx, oracle, X, q, mask, ctx, tail_ones=True):
    """host form and device form (odd address, ones around the bitmap) against the oracle; k = 2048: the labels are the set"""
    n = mask.size
    bits = bc.pack(mask)
    if tail_ones:
        bits = ic.with_tail_ones(bits, n)
    ol, od = ic.search_bitmap(oracle, L2, q, X[:n], 2048, bits)
    vis = np.flatnonzero(mask)
    assert np.array_equal(np.sort(ol[0][ol[0] >= 0]), vis)
    odd = np.full(bits.size + 3, 0xFF, np.uint8)                # a host bitmap at an odd byte address, ones around it
    off = 1 if odd.ctypes.data % 2 == 0 else 2
    odd[off:off + bits.size] = bits
    host = odd[off:off + bits.size]
    assert host.ctypes.data % 2 == 1
    for view in (host, bits):
        lab, dist = idx.SearchBatch(q, 2048, bitmap=view)
        assert_same(lab, dist, ol, od, f"{ctx} (host)")
    for offset in (1, 3):
        lab, dist = dev_search(idx, q, 2048, bits, n, offset=offset)
        assert_same(lab, dist, ol, od, f"{ctx} (device, offset {offset})")


def test_kernel_edges_growing_one_index(oracle, small):
    gpu_or_skip()
    X, q = small
    idx = new_index(8, L2)
    try:
        have = 0
        for n in ic.EDGE_N:
            idx.Add(None, X[have:n])
            have = n
            assert idx.ntotal == n
            rng = np.random.default_rng(n)
            first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            first[0], last[n - 1] = 1, 1
            cases = {"random half": (rng.random(n) < 0.5).astype(np.uint8), "first row alone": first, "last row alone": last,
                     "all ones": np.ones(n, np.uint8), "all but the last": 1 - last}
            for name, mask in cases.items():
                if mask.sum() > 2048:
                    mask = mask.copy()
                    mask[1] = 0  # (k = 2048 returns the whole visible set only while it has at most 2048 rows)
                _check_small(idx, oracle, X, q, mask, f"n {n} '{name}'")
            assert idx.nvisible() == n
    finally:
        idx.Close()


def test_an_empty_block_between_two_that_have_rows(oracle):
    gpu_or_skip()
    rng = np.random.default_rng(104)
    n = 3 * ic.BLOCK + 5
    X, q = rng.random((n, 8), dtype=F), rng.random((1, 8), dtype=F)
    mask = ic.block_gap_mask(n, rng)
    idx = new_index(8, L2)
    try:
        idx.Add(None, X)
        _check_small(idx, oracle, X, q, mask, "block gap")
    finally:
        idx.Close()


# 5 ---- AND with the handle's own mask, and untouched state ----------------------------------------------------------
@pytest.mark.parametrize("state", ["selective filter", "filter above 95 %", "removed rows", "filter and removed rows"])
def test_and_with_the_handle_mask_and_untouched_state(oracle, corpus, state):
    gpu_or_skip()
    X, Q = corpus
    Q = Q[:64]
    n, k = X.shape[0], 10
    rng = np.random.default_rng(len(state))
    idx = new_index(X.shape[1], L2)
    try:
        idx.Add(None, X)
        also = np.ones(n, np.uint8)
        if "filter" in state:
            filt = rc.byte_mask(rng, n, 0.97 if "95" in state else 0.1)
            filt[n // 3] = 0                                      # query 0's nearest neighbour is hidden by the handle
            idx.set_filter(filt)
            also &= (filt != 0).astype(np.uint8)
        if "removed" in state:
            gone = rng.choice(n, 700, replace=False)
            gone[0] = n // 3
            assert idx.remove_rows(gone) == np.unique(gone).size
            also[gone] = 0
        nvis, nlive = idx.nvisible(), idx.nlive()
        assert nvis == int(also.sum())
        plain = idx.SearchBatch(Q, k)
        assert_same(*plain, *oracle.search_batch(L2, Q, X, k, mask=also, nthreads=16), f"{state}: plain")
        for name, mask in (("all ones", np.ones(n, np.uint8)), ("50 %", (rng.random(n) < 0.5).astype(np.uint8)),
                           ("1 %", (rng.random(n) < 0.01).astype(np.uint8))):
            mask[n // 3] = 1                                      # a bit set for a hidden / removed row does not resurrect it
            bits = bc.pack(mask)
            ol, od = ic.search_bitmap(oracle, L2, Q, X, k, bits, also=also)
            assert n // 3 not in ol
            for nq in (1, 64):
                assert_same(*idx.SearchBatch(Q[:nq], k, bitmap=bits), ol[:nq], od[:nq], f"{state}: bitmap '{name}' nq {nq}")
            assert_same(*dev_search(idx, Q, k, bits, n), ol, od, f"{state}: bitmap '{name}' device form")
            assert idx.nvisible() == nvis and idx.nlive() == nlive
            assert_same(*idx.SearchBatch(Q, k), *plain, f"{state}: plain after bitmap '{name}'")
    finally:
        idx.Close()


# 6 ---- the shared sample map ----------------------------------------------------------------------------------------
def test_the_shared_sample_map_is_neither_read_nor_published(oracle):
    """200,000 x 32, 64 queries, k = 10: the plain batch (200,000 positions) and the bitmap batch at 10 % (a row list of 20,000)
    both lie above the 16,384 positions from which sample_plan is on, and a 64-query batch on the narrow tiles scores its sample
    through sample_map -- the handle's shared map for the plain batch, the workspace's own for the call's view"""
    gpu_or_skip()
    rng = np.random.default_rng(106)
    n, d, k = 200000, 32, 10
    X, Q = rng.random((n, d), dtype=F), rng.random((64, d), dtype=F)
    mask = rc.exact_count_mask(rng, n, n // 10)
    bits = bc.pack(mask)
    ol, od = oracle.search_batch(L2, Q, X, k, nthreads=16)
    bl, bd = ic.search_bitmap(oracle, L2, Q, X, k, bits)
    a = new_index(d, L2)
    b = new_index(d, L2)
    try:
        a.Add(None, X)
        first = a.SearchBatch(Q, k)
        assert_same(*first, ol, od, "plain batch")
        assert_same(*a.SearchBatch(Q, k, bitmap=bits), bl, bd, "bitmap batch behind a plain one")
        assert_same(*a.SearchBatch(Q, k), *first, "plain batch again")
        b.Add(None, X)                                            # a fresh index, the other order
        assert_same(*b.SearchBatch(Q, k, bitmap=bits), bl, bd, "bitmap batch first")
        assert_same(*b.SearchBatch(Q, k), ol, od, "plain batch behind a bitmap one")
    finally:
        a.Close()
        b.Close()


# 7 ---- ids ----------------------------------------------------------------------------------------------------------
def test_labels_are_ids(oracle, corpus):
    gpu_or_skip()
    X, Q = corpus
    n, k = X.shape[0], 10
    ids = np.arange(n, dtype=np.int64)[::-1] * 3 + (1 << 33)
    mask = rc.byte_mask(np.random.default_rng(7), n, 0.1)
    bits = bc.pack(mask)
    idx = new_index(X.shape[1], L2)
    try:
        idx.Add(ids, X)
        ol, od = ic.search_bitmap(oracle, L2, Q[:64], X, k, bits, ids=ids)
        assert ol.min() >= (1 << 33)
        for nq in (1, 64):
            assert_same(*idx.SearchBatch(Q[:nq], k, bitmap=bits), ol[:nq], od[:nq], f"ids nq {nq}")
        l1, d1 = idx.Search(Q[4], k, bitmap=bits)
        assert np.array_equal(l1, ol[4]) and np.array_equal(d1, od[4])
    finally:
        idx.Close()


# 8 ---- concurrency --------------------------------------------------------------------------------------------------
def test_concurrent_bitmap_calls_beside_combined_plain_calls(corpus):
    """Eight threads, each with its own bitmap and 50 single-query calls, beside plain single-query calls with combining on:
    every answer equals the one the same request got alone, and the plain calls were still combined.  The plain callers are
    FOUR threads: the combiner serves up to two callers at once on two lanes and queues only the third (lb_combine.h), so
    two plain threads alone are never combined, by design."""
    gpu_or_skip()
    X, Q = corpus
    n, k, per, plain_threads, plain_calls = X.shape[0], 10, 50, 4, 200
    idx = new_index(X.shape[1], L2)
    try:
        idx.Add(None, X)
        idx.set_search_combining(True)
        rng = np.random.default_rng(8)
        dens = (0.01, 0.1, 0.5, 0.9, 0.96, 1.0, 0.3, 0.001)
        bitmaps = [bc.pack((rng.random(n) < p).astype(np.uint8)) for p in dens]
        alone_b = [[idx.SearchBatch(Q[(t * per + i) % Q.shape[0]][None, :], k, bitmap=bitmaps[t]) for i in range(per)] for t in range(8)]
        alone_p = [idx.SearchBatch(Q[i][None, :], k) for i in range(per)]
        before = idx.combining_stats
        wrong, errors = [], []
        start = threading.Barrier(8 + plain_threads)

        def with_bitmap(t):
            try:
                start.wait()
                for i in range(per):
                    lab, dist = idx.SearchBatch(Q[(t * per + i) % Q.shape[0]][None, :], k, bitmap=bitmaps[t])
                    if not (np.array_equal(lab, alone_b[t][i][0]) and np.array_equal(dist, alone_b[t][i][1])):
                        wrong.append(("bitmap", t, i))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        def plain(t):
            try:
                start.wait()
                for j in range(plain_calls):
                    i = (j + t) % per
                    lab, dist = idx.SearchBatch(Q[i][None, :], k)
                    if not (np.array_equal(lab, alone_p[i][0]) and np.array_equal(dist, alone_p[i][1])):
                        wrong.append(("plain", t, j))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=with_bitmap, args=(t,)) for t in range(8)]
        threads += [threading.Thread(target=plain, args=(t,)) for t in range(plain_threads)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors and not wrong, (errors, wrong[:5])
        after = idx.combining_stats
        assert after[0] > before[0] and after[1] - before[1] >= 2 * (after[0] - before[0]), (before, after)
        assert after[1] - before[1] <= plain_threads * plain_calls        # no bitmap call was ever part of a combined batch
        assert idx.nvisible() == n
    finally:
        idx.Close()


# 9 ---- the device form on a caller's stream -------------------------------------------------------------------------
def test_device_form_on_a_callers_stream(oracle, corpus, filled):
    import torch
    X, Q = corpus
    n, k = X.shape[0], 10
    Q = Q[:64]
    mask = rc.byte_mask(np.random.default_rng(9), n, 0.5)
    bits = bc.pack(mask)
    nb = bits.size
    whole = torch.full((nb + 7,), 0xFF, dtype=torch.uint8, device="cuda")
    whole[3:3 + nb] = torch.from_numpy(bits).cuda()
    d_bits = whole[3:3 + nb]                                       # a torch uint8 tensor sliced to an odd offset
    assert d_bits.data_ptr() % 2 == 1
    dQ = torch.from_numpy(np.array(Q)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dD = torch.empty((64, k), dtype=torch.float32, device="cuda")
        dL = torch.empty((64, k), dtype=torch.int64, device="cuda")
        filled.search_device(64, dQ.data_ptr(), k, dD.data_ptr(), dL.data_ptr(), stream=s.cuda_stream, d_bitmap=d_bits.data_ptr(), nbits=n)
        chained_l, chained_d = dL + 1, dD * 2                      # chained on the same stream
    s.synchronize()
    ol, od = ic.search_bitmap(oracle, L2, Q, X, k, bits)
    assert_same(dL.cpu().numpy(), dD.cpu().numpy(), ol, od, "device form on a caller's stream")
    assert np.array_equal(chained_l.cpu().numpy(), ol + 1) and np.array_equal(chained_d.cpu().numpy(), od * F(2))
    assert filled.nvisible() == n


# 10 ---- arguments ---------------------------------------------------------------------------------------------------
def test_arguments(oracle, corpus):
    gpu_or_skip()
    from longbow_amd import gpu
    X, Q = corpus
    X, Q = X[:3000], Q[:5]
    n, k, nq = X.shape[0], 10, Q.shape[0]
    idx = new_index(X.shape[1], L2)
    empty = new_index(X.shape[1], L2)
    f16 = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=X.shape[1], DataType=gpu.DataType.Float16))
    try:
        idx.Add(None, X)
        lib = idx._lib
        err = lambda h=idx: lib.lb_gpu_last_error(h._h).decode()
        bits = np.full(bc.nbytes(n) + 8, 0xFF, np.uint8)
        host = lib.lb_gpu_index_search_bitmap_ctx

        def call(fn, h, q, bitmap, nbits, ctx=None):
            dist = np.full((nq, k), -3.0, F)
            lab = np.full((nq, k), -9, np.int64)
            return fn(h._h, nq, q.ctypes.data, k, bitmap, nbits, dist.ctypes.data, lab.ctypes.data, ctx), dist, lab

        want = idx.SearchBatch(Q, k)
        for nbits in (n - 1, n + 1):                              # one short and one long: both numbers in last_error
            rcode, dist, lab = call(host, idx, Q, bits.ctypes.data, nbits)
            assert rcode == INVALID and (dist == -3.0).all() and (lab == -9).all()
            assert "bitmap" in err() and str(nbits) in err() and str(n) in err(), err()
        with pytest.raises(ValueError):
            idx.SearchBatch(Q, k, bitmap=bits[:bc.nbytes(n) - 1])
        with pytest.raises(ValueError):
            idx.SearchBatch(Q, k, bitmap=bits[:bc.nbytes(n) + 1])
        # the plain entry point's checks come first: k = 0, and nq == 0 is LB_OK whatever the bitmap says
        dist = np.full((nq, k), -3.0, F)
        lab = np.full((nq, k), -9, np.int64)
        assert host(idx._h, nq, Q.ctypes.data, 0, bits.ctypes.data, n + 1, dist.ctypes.data, lab.ctypes.data, None) == INVALID
        assert host(idx._h, 0, Q.ctypes.data, k, bits.ctypes.data, n + 1, dist.ctypes.data, lab.ctypes.data, None) == OK
        # a bitmap of the old length after a later Add
        old = gpu.pack_bitmap(np.ones(n, np.uint8))[0]
        idx.Add(None, X[:5])
        rcode, dist, lab = call(host, idx, Q, old.ctypes.data, n)
        assert rcode == INVALID and str(n) in err() and str(n + 5) in err() and (lab == -9).all()
        n5 = n + 5
        # a fired context: LB_ERR_CANCELLED, and the next call is fine
        c = gpu.Cancel()
        c.fire()
        rcode, dist, lab = call(host, idx, Q, bits.ctypes.data, n5, c._h)
        assert rcode == CANCELLED
        with pytest.raises(gpu.Canceled):
            idx.SearchBatch(Q, k, ctx=c, bitmap=bits[:bc.nbytes(n5)])
        X5 = np.concatenate([X, X[:5]])
        mask = (np.arange(n5) % 3 == 0).astype(np.uint8)
        assert_same(*idx.SearchBatch(Q, k, bitmap=bc.pack(mask)), *ic.search_bitmap(oracle, L2, Q, X5, k, bc.pack(mask)), "after a cancelled call")
        c.close()
        # a NULL bitmap equals the plain call, whatever nbits says
        want = idx.SearchBatch(Q, k)
        rcode, dist, lab = call(host, idx, Q, None, -5)
        assert rcode == OK
        assert_same(lab, dist, *want, "NULL bitmap")
        # an empty index: all padding; a bitmap of the wrong length is still refused
        rcode, dist, lab = call(host, empty, Q, bits.ctypes.data, 0)
        assert rcode == OK and (lab == -1).all() and (dist == FLT_MAX).all()
        assert call(host, empty, Q, bits.ctypes.data, 8)[0] == INVALID
        lab, dist = empty.SearchBatch(Q, k, bitmap=np.zeros(0, np.uint8))
        assert (lab == -1).all() and (dist == FLT_MAX).all()
        # an entry point of another element type names the index's type
        Qh = Q.astype(np.float16)
        Q8 = np.zeros(Q.shape, np.int8)
        rcode, dist, lab = call(lib.lb_gpu_index_search_f16_bitmap_ctx, idx, Qh, bits.ctypes.data, n5)
        assert rcode == INVALID and "float32" in err() and (lab == -9).all()
        rcode, dist, lab = call(lib.lb_gpu_index_search_i8_bitmap_ctx, idx, Q8, bits.ctypes.data, n5)
        assert rcode == INVALID and "float32" in err() and (lab == -9).all()
        f16.Add(None, X.astype(np.float16))
        rcode, dist, lab = call(host, f16, Q, bits.ctypes.data, n)
        assert rcode == INVALID and "float16" in err(f16) and (lab == -9).all()
        dist = np.full((nq, k), -3.0, F)
        lab = np.full((nq, k), -9, np.int64)
        assert lib.lb_gpu_index_search_i8_bitmap_device_ctx(f16._h, nq, Q8.ctypes.data, k, bits.ctypes.data, n, dist.ctypes.data,
                                                            lab.ctypes.data, None, None) == INVALID
        assert "float16" in err(f16) and (lab == -9).all()
    finally:
        idx.Close()
        empty.Close()
        f16.Close()
