"""Row filters on the PQ handle (lb_gpu_pq_set_filter, _filter_int64 / _float32, _nvisible) on the GPU.  The expected result
everywhere is the C oracle on the visible subset (tests/pq_filter_cases.py: subset_search, pinned on the CPU by
tests/test_pq_filter_semantics.py together with the preconditions of the cases below); labels and distances are compared for
equality, and lb_gpu_pq_last_search_stats shows which list form served the queries.

Under a filter a search walks the list of visible rows (kernels_pq_list.hip): fewer than 65,536 visible rows take the boot chunk
and the chunk schedule of the list exact scan; from there on the sampled threshold over the list and the list prefilter (pairs
of queries share a pass where M / 16 is 1, 2, 3, 4 or 6 and the codes are 16-B aligned; M = 128 runs aligned single passes, any
other M the generic single form); with the prefilter off the list exact scan admits over the whole list."""
import threading

import numpy as np
import pytest

from tests import code_filter_cases as cf
from tests import pq_filter_cases as pc
from tests import row_view_cases as rv
from tests.gpu_util import gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = pc.FLT_MAX


def _enc(cb, codes=None):
    gpu_or_skip()
    from longbow_amd import pq
    enc = pq.PQEncoder(pq.serialize_codebooks(cb))
    if codes is not None:
        enc.add_codes(codes)
    return enc


def _check(oracle, enc, cb, codes, Q, mask, k, ctx, want=None):
    lab, dist = enc.Search(Q, k)
    wlab, wdist = want if want is not None else pc.subset_search(oracle, cb, codes, Q, mask, k)
    assert np.array_equal(lab, wlab), f"labels differ {ctx}: {np.argwhere(lab != wlab)[:5]} stats {enc.last_search_stats}"
    assert np.array_equal(dist, wdist, equal_nan=True), f"distances differ {ctx}: stats {enc.last_search_stats}"
    return lab, dist


# ---- A. one boot chunk: every mask, aligned MCH 1 / 3 / 6 and the generic form -----------------------------------------------
@pytest.mark.parametrize("k", (1, 10, 100))
@pytest.mark.parametrize("dims,M", pc.SHAPES)
def test_masked_search_equals_the_oracle_on_the_visible_rows(oracle, dims, M, k):
    cb, codes, Q = pc.corpus(dims, M, pc.N)
    enc = _enc(cb, codes)
    rng = np.random.default_rng(dims + k)
    for name, mask in cf.masks(pc.N, k, rng).items():
        enc.set_filter(mask)
        nvis = int(np.count_nonzero(mask))
        assert enc.nvisible() == nvis and enc.ntotal == pc.N, name
        wlab, wdist = pc.subset_search(oracle, cb, codes, Q, mask, k)  # (5 queries; a smaller batch is its first rows)
        for nq in (1, 2, 5):
            lab, dist = _check(oracle, enc, cb, codes, Q[:nq], mask, k, f"{name}, {dims}/{M}, nq {nq}, k {k}", (wlab[:nq], wdist[:nq]))
            assert enc.last_search_stats[:4] == (0, 0, 0, 0), name  # no sampled plan below 65,536 visible rows
            if name.endswith("rows spread") or name == "all-zero":  # the padding: the visible rows first, then -1 / FLT_MAX
                have = min(k, nvis)
                assert (lab[:, :have] >= 0).all() and (lab[:, have:] == -1).all() and (dist[:, have:] == FLT_MAX).all(), (name, nq)
    enc.Close()


# ---- B. several chunks of the list ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,M", pc.FEW)
def test_a_list_of_several_chunks(oracle, dims, M):
    cb, codes, Q = pc.corpus(dims, M, pc.N_CHUNKS, nq=3)
    mask = pc.half_mask(pc.N_CHUNKS)
    enc = _enc(cb, codes)
    enc.set_filter(mask)
    assert pc.BOOT_POSITIONS < enc.nvisible() == np.count_nonzero(mask) < 65536
    for k in (10, 300):
        _check(oracle, enc, cb, codes, Q, mask, k, f"{dims}/{M} k {k}")
        assert enc.last_search_stats[0] == 0
    enc.Close()


# ---- C. the schedule that cannot overflow ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (16, 5))
def test_decreasing_distances_force_the_safe_schedule(oracle, M):
    """pc.case_c: every position behind the 8192-position boot chunk beats its threshold, the 11,808 of the next chunk overflow
    the 8192-entry list and both queries are redone on the schedule that cannot overflow (stats[5])"""
    cb, codes, Q, mask = pc.case_c(M)
    enc = _enc(cb, codes)
    enc.set_filter(mask)
    _check(oracle, enc, cb, codes, Q, mask, 100, f"M {M}")
    stats = enc.last_search_stats
    assert stats[5] == 2, stats
    enc.Close()


# ---- D. sampled threshold over the list and the list prefilter -------------------------------------------------------------------
@pytest.mark.parametrize("mask_name", ("half", "thirds"))
@pytest.mark.parametrize("dims,M", ((32, 16), (768, 96), (60, 5)))
def test_sampled_plan_under_a_list(oracle, dims, M, mask_name):
    cb, codes, Q = pc.corpus(dims, M, pc.N_BIG)
    mask = pc.half_mask(pc.N_BIG) if mask_name == "half" else pc.third_mask(pc.N_BIG)
    k, nq = 100, 5
    enc = _enc(cb, codes)
    enc.set_filter(mask)
    assert enc.nvisible() == np.count_nonzero(mask) >= 65536
    want = pc.subset_search(oracle, cb, codes, Q, mask, k)
    _check(oracle, enc, cb, codes, Q, mask, k, f"{dims}/{M} {mask_name}", want)
    stats = enc.last_search_stats
    print(f"sampled plan under a list {dims}/{M} {mask_name}: last_search_stats {stats}")
    assert stats[0] == nq and stats[1] == 0, stats
    if M % 16 == 0:
        assert stats[2] == 4 and stats[3] == 1, stats  # two pairs and a single
    else:
        assert stats[2] == 0 and stats[3] == 5, stats  # the generic form: one query per pass
    enc.set_prefilter(False)  # the list exact scan in admission mode over the whole list
    _check(oracle, enc, cb, codes, Q, mask, k, f"{dims}/{M} {mask_name}, prefilter off", want)
    stats = enc.last_search_stats
    assert stats[0] == nq and stats[2] == stats[3] == 0, stats
    enc.Close()


def test_k_beyond_the_sampled_plan_under_a_list(oracle):
    cb, codes, Q = pc.corpus(32, 16, pc.N_BIG)
    mask = pc.half_mask(pc.N_BIG)
    enc = _enc(cb, codes)
    enc.set_filter(mask)
    _check(oracle, enc, cb, codes, Q[:2], mask, 1500, "k 1500")
    assert enc.last_search_stats[:4] == (0, 0, 0, 0)
    enc.Close()


# ---- E. ties at that size ----------------------------------------------------------------------------------------------------------
def test_ties_under_a_list_at_the_sampled_size(oracle):
    cb, codes, Q, mask = pc.case_e()
    enc = _enc(cb, codes)
    enc.set_filter(mask)
    _check(oracle, enc, cb, codes, Q, mask, 100, "ties")
    enc.Close()


# ---- F. duplicates across the list's tile and workgroup boundaries ---------------------------------------------------------------
@pytest.mark.parametrize("dims,M", ((32, 16), (60, 5)))
def test_duplicates_across_the_boundaries_of_the_list(oracle, dims, M):
    """A block of rows at distance 0 whose visible members straddle list positions 63 / 64 (a wave's tile) and, in a second
    corpus, the end of a workgroup's run of ADC_LIST_WAVES * 64 positions; the hidden rows between them are duplicates too and
    must not come back"""
    for boundary in sorted({64, pc.list_waves() * 64}):
        cb, codes, Q, mask, block = pc.case_f(dims, M, boundary)
        enc = _enc(cb, codes)
        enc.set_filter(mask)
        for k in (6, 12, 20):
            lab, dist = _check(oracle, enc, cb, codes, Q, mask, k, f"{dims}/{M} boundary {boundary} k {k}")
            m = min(k, 12)
            assert np.array_equal(lab[0, :m], block[:m]) and (dist[0, :m] == 0).all()
        enc.Close()


# ---- G. the prefilter declines ---------------------------------------------------------------------------------------------------
def test_prefilter_declines_under_a_list(oracle):
    cb0, cb, codes, Q, mask = pc.case_g()
    vis = np.flatnonzero(mask)
    k = 10
    enc = _enc(cb0, codes)  # constant sub-tables: every distance ties, the candidate buffer overflows
    enc.set_filter(mask)
    lab, dist = _check(oracle, enc, cb0, codes, Q[:1], mask, k, "constant tables")
    stats = enc.last_search_stats
    assert np.array_equal(lab[0], vis[:k]) and len(np.unique(dist)) == 1
    assert stats[0] == 1 and stats[4] + stats[5] >= 1, stats
    enc.Close()
    enc = _enc(cb, codes)  # a query with an infinite component: refused on the device, redone on the exact schedule
    enc.set_filter(mask)
    _check(oracle, enc, cb, codes, Q, mask, k, "infinite component")
    stats = enc.last_search_stats
    assert stats[0] == 2 and stats[4] + stats[5] >= 1, stats
    enc.Close()


# ---- H. life cycle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,M", ((32, 16), (60, 5)))
def test_filter_life_cycle(oracle, dims, M):
    from longbow_amd import _lib
    cb, codes, Q = pc.corpus(dims, M, pc.N)
    k = 10
    rng = np.random.default_rng(3)
    enc = _enc(cb, codes)
    assert enc.nvisible() == pc.N
    first = enc.Search(Q, k)
    mask = rv.byte_mask(rng, pc.N, 0.3)
    enc.set_filter(mask)
    _check(oracle, enc, cb, codes, Q, mask, k, "set")
    # what addresses rows directly ignores the filter
    hidden = np.flatnonzero(mask == 0)[:7]
    assert np.array_equal(enc.get_codes(int(hidden[0]), 1), codes[hidden[:1]])
    table = enc.BuildADCTable(Q[1])
    every = np.full(pc.N, -1, F)
    enc.ADCDistanceBatch(table, every)
    want_every = oracle.adc_batch(oracle.build_adc_table(cb, Q[1]), codes)
    assert np.array_equal(every, want_every)
    assert np.array_equal(enc.Rerank(Q[1], hidden)[0], want_every[hidden])
    # a mask or a column of the wrong length is refused and the old filter still holds
    for bad in (mask[:-1], np.concatenate([mask, mask[:1]])):
        with pytest.raises(_lib.LongbowGPUError) as e:
            enc.set_filter(bad)
        assert e.value.code == 1 and "rows" in str(e.value)
    with pytest.raises(_lib.LongbowGPUError) as e:
        enc.filter_column(np.zeros(pc.N - 1, np.int64), 0, rv.EQ)
    assert e.value.code == 1
    assert enc.nvisible() == np.count_nonzero(mask)
    _check(oracle, enc, cb, codes, Q, mask, k, "after the refusals")
    # rows added under a filter are visible, across a growth of the buffers too (5003 -> 9003 rows)
    more = pc.codes_of(rng, 4000, M, (dims, M) in pc.FEW)
    more[:3] = enc.Encode(Q[:3])
    enc.add_codes(more)
    both, mask2 = np.concatenate([codes, more]), np.concatenate([mask, np.ones(4000, np.uint8)])
    assert enc.ntotal == pc.N + 4000 and enc.nvisible() == np.count_nonzero(mask) + 4000
    lab, _ = _check(oracle, enc, cb, both, Q, mask2, k, "after add_codes")
    assert lab[0, 0] == pc.N and lab[1, 0] == pc.N + 1  # the added rows are found: each carries its query's nearest code
    assert np.array_equal(enc.get_codes(pc.N - 2, 4), both[pc.N - 2:pc.N + 2])
    # clearing returns the unfiltered result of the grown index
    enc.set_filter(None)
    assert enc.nvisible() == enc.ntotal
    _check(oracle, enc, cb, both, Q, np.ones(both.shape[0], np.uint8), k, "cleared")
    enc.Close()
    # a handle that was filtered and then cleared returns the first unfiltered result bit for bit
    enc = _enc(cb, codes)
    enc.set_filter(mask)
    enc.set_filter(None)
    again = enc.Search(Q, k)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    enc.Close()
    # a filter set on an empty handle covers what is added later
    enc = _enc(cb)
    enc.set_filter(np.zeros(0, np.uint8))
    assert enc.nvisible() == 0
    lab, dist = enc.Search(Q, k)
    assert (lab == -1).all() and (dist == FLT_MAX).all()
    enc.add_codes(codes[:300])
    assert enc.nvisible() == 300
    _check(oracle, enc, cb, codes[:300], Q, np.ones(300, np.uint8), k, "filter set on an empty handle")
    enc.Close()


def test_vectors_added_on_the_device_under_a_filter_are_visible(oracle):
    import torch
    dims, M, n, k = 32, 16, 700, 20
    rng = np.random.default_rng(9)
    cb = pc.codebooks(rng, dims, M)
    X = rng.random((n, dims), dtype=F)
    Q = rng.random((3, dims), dtype=F)
    mask = rv.byte_mask(rng, n, 0.5)
    enc = _enc(cb)
    dX = torch.from_numpy(X).cuda()
    enc.add_vectors_device(n, dX.data_ptr())
    enc.set_filter(mask)
    enc.add_vectors_device(50, dX.data_ptr())
    assert enc.ntotal == n + 50 and enc.nvisible() == np.count_nonzero(mask) + 50
    codes = enc.get_codes()
    assert np.array_equal(codes[n:], codes[:50])
    _check(oracle, enc, cb, codes, Q, np.concatenate([mask, np.ones(50, np.uint8)]), k, "add_vectors_device")
    enc.Close()


# ---- I. predicates evaluated on the device -----------------------------------------------------------------------------------------
def test_filter_column_equals_the_restated_predicate(oracle):
    dims, M = 32, 16
    n, k = rv.EDGE_N, 10
    cb, codes, Q = pc.corpus(dims, M, n)
    rng = np.random.default_rng(17)
    icol, fcol = rv.int64_edge_column(n), rv.float32_edge_column(n)
    ivalid, fvalid = rng.random(n) < 0.8, rng.random(n) < 0.8
    enc = _enc(cb, codes)
    # combine on a handle without a filter replaces the mask
    enc.filter_column(icol, 2 ** 32, rv.GE, valid=rv.validity_bitmap(ivalid, 3), validity_offset=3, combine=True)
    m1 = rv.predicate(icol, 2 ** 32, rv.GE, ivalid)
    assert 0 < m1.sum() < n and enc.nvisible() == m1.sum()
    _check(oracle, enc, cb, codes, Q, m1, k, "int64 GE, combine on no filter")
    # combine 0 replaces, combine 1 ANDs into it
    enc.filter_column(fcol, 0.25, rv.LE, valid=rv.validity_bitmap(fvalid, 5), validity_offset=5, combine=False)
    m2 = rv.predicate(fcol, 0.25, rv.LE, fvalid)
    assert 0 < m2.sum() < n and enc.nvisible() == m2.sum()
    _check(oracle, enc, cb, codes, Q, m2, k, "float32 LE, replace")
    enc.filter_column(icol, 5, "!=", valid=rv.validity_bitmap(ivalid, 3), validity_offset=3, combine=True)
    m3 = rv.and_bytes(m2, rv.predicate(icol, 5, rv.NEQ, ivalid))
    assert 0 < m3.sum() < m2.sum() and enc.nvisible() == m3.sum()
    _check(oracle, enc, cb, codes, Q, m3, k, "int64 NEQ, combined")
    with pytest.raises(TypeError):
        enc.filter_column(icol.astype(np.int32), 5, rv.EQ)
    enc.Close()


# ---- J. combined concurrent host searches ------------------------------------------------------------------------------------------
def test_concurrent_searches_under_a_filter_are_combined_exactly(oracle):
    dims, M, k = 32, 16, 10
    cb, codes, _ = pc.corpus(dims, M, pc.N)
    Q = np.random.default_rng(8).random((8, dims), dtype=F)
    mask = pc.half_mask(pc.N)
    wlab, wdist = pc.subset_search(oracle, cb, codes, Q, mask, k)
    enc = _enc(cb, codes)
    enc.set_filter(mask)
    got = [None] * 8
    start = threading.Barrier(8)

    def one(i):
        start.wait()
        got[i] = enc.Search(Q[i], k)

    threads = [threading.Thread(target=one, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i in range(8):
        assert got[i] is not None, i
        assert np.array_equal(got[i][0][0], wlab[i]) and np.array_equal(got[i][1][0], wdist[i]), i
    enc.Close()
