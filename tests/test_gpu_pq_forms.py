"""Every ADC search and PQ codec kernel form against the oracle, bit for bit, with lb_gpu_pq_last_search_stats proving
which form served each query (a results-only test cannot see a broken prefilter: the exact redo would hide it).

Which form a batch takes (launchers in kernels_pq2.hip, the walk in pq.hip: PqSearch::walk / sampled_group /
prefilter_group), for a sampled plan with the prefilter on and a corpus of >= 4096 rows:

    M            four-query form              two-query form               single form
    16 32 48 64  <M/16, 16>: tables M KiB +   <M/16, 16, 2>: M/2 + M KiB   <M/16, 16>: M/4 + M KiB
                 staging M KiB = 32..128 KiB  = 24 .. 96 KiB               = 20 .. 80 KiB
    96           <6, 10>: 96 + 60 KiB         <6, 16, 2>: 48 + 96 KiB      <6, 16>: 24 + 96 KiB
                 = 159,744 B <= 163,840 B     = 147,456 B                  = 122,880 B
    128          no case                      no case                      <8, 10>: 32 + 80 KiB = 114,688 B
    80 112 144   no case                      no case                      no case -> generic kernel
    M % 16 != 0  refused (not vectorisable)   refused                      generic kernel (M * 256 B of LDS)

(staging = WAVES x 64 rows x M bytes; every launcher refuses a form above 160 KiB = 163,840 B.)
A batch of nq queries is walked as quads while four remain, then a pair while two remain, then a single; a quad or a
pair whose M has no shared form runs single passes and counts under "single".  So nq = 7 gives (7, 4, 2, 1, 0, 0) at
M = 96 and (7, 0, 0, 7, 0, 0) at M = 128.  With the prefilter switched off only the plan is counted: (nq, 0, 0, 0, 0, 0);
below 65,536 rows (or when k is too large for the sample) there is no sampled plan: all zero."""
import numpy as np
import pytest

from tests import adc_bound as ab
from tests.gpu_util import gpu_or_skip
from tests.adc_bound import family, wrong_survivor_corpus

pytestmark = pytest.mark.gpu
F = np.float32
SHARED_FORMS = (1, 2, 3, 4, 6)  # M / 16 with a `case` in launch_adc_prefilter4 and launch_adc_prefilter2
LDS_LIMIT = 160 * 1024
N_GRID = 66001                  # >= 65,536 (sampled plan), 66001 % 64 == 17 (the clamped tail tile runs)


def expected_stats(M, nq, sampled=True, prefilter=True):
    if not sampled:
        return (0, 0, 0, 0, 0, 0)
    if not prefilter:
        return (nq, 0, 0, 0, 0, 0)
    shared = M % 16 == 0 and M // 16 in SHARED_FORMS
    has4 = shared and M * 1024 + (10 if M == 96 else 16) * 64 * M <= LDS_LIMIT
    has2 = shared and 2 * M * 256 + 16 * 64 * M <= LDS_LIMIT
    four = two = one = 0
    q = 0
    while q < nq:
        if q + 3 < nq:
            if has4:
                four += 4
            elif has2:
                two += 4
            else:
                one += 4
            q += 4
        elif q + 1 < nq:
            if has2:
                two += 2
            else:
                one += 2
            q += 2
        else:
            one += 1
            q += 1
    return (nq, four, two, one, 0, 0)


def test_expected_stats_examples():
    assert expected_stats(96, 7) == (7, 4, 2, 1, 0, 0)
    assert expected_stats(128, 7) == (7, 0, 0, 7, 0, 0)
    assert expected_stats(16, 4) == (4, 4, 0, 0, 0, 0)
    assert expected_stats(20, 2) == (2, 0, 0, 2, 0, 0)
    assert expected_stats(16, 6) == (6, 4, 2, 0, 0, 0)
    assert expected_stats(128, 3) == (3, 0, 0, 3, 0, 0)


def _encoder(cb, codes=None):
    from longbow_amd import pq
    enc = pq.PQEncoder(pq.serialize_codebooks(cb))
    if codes is not None:
        enc.add_codes(codes)
    return enc


def _oracle_lists(oracle, cb, Q, codes, k):
    out = []
    for q in Q:
        table = oracle.build_adc_table(cb, q)
        d = oracle.adc_batch(table, codes)
        oi, od, _ = oracle.topk_canonical(d, k)
        out.append((oi, od, d, table))
    return out


def _assert_lists(lab, dist, want, ctx):
    for b in range(lab.shape[0]):
        assert np.array_equal(lab[b], want[b][0]), (ctx, b, "labels")
        assert np.array_equal(dist[b], want[b][1], equal_nan=True), (ctx, b, "distances")


def grid_case(oracle, M, k=10, nq=7):
    """inputs of the form grid at this M, with the precondition of a search without any redo ASSERTED on the oracle's
    distances: the sampled tau admits at least k rows and no more than the list holds, the byte bound loses none of
    them and its survivors fit the candidate buffer"""
    rng = np.random.default_rng(9000 + M)
    sub = 2
    cb = rng.random((M, 256, sub), dtype=F)
    codes = rng.integers(0, 256, (N_GRID, M), dtype=np.uint8)
    Q = rng.random((nq, M * sub), dtype=F)
    want = _oracle_lists(oracle, cb, Q, codes, k)
    cnt, m, stride, cap = ab.plan(N_GRID, k)
    assert cnt == 8192 and stride == 256 and cap == 16384 and m <= 32
    for b, (_, _, d, table) in enumerate(want):
        tau = ab.sampled_tau(d, cnt, m)
        admitted = int((d <= tau).sum())
        assert k <= admitted <= cap, (M, b, admitted)
        qt, s_tau, ok = ab.quantise(table.reshape(M, 256), tau)
        S = ab.byte_sums(qt, codes)
        assert ok == 1 and not ((d <= tau) & (S > s_tau)).any(), (M, b)
        assert int((S <= s_tau).sum()) <= ab.CAND_CAP, (M, b)
    return cb, codes, Q, want


@pytest.mark.parametrize("M", [16, 32, 48, 64, 80, 96, 112, 128, 144, 159, 20, 100])
def test_form_grid(oracle, M):
    """nq = 1 .. 7 at every M (every group boundary: pair + single, quad + single, quad + pair, quad + pair + single):
    oracle equality, batch == single == prefilter off, the split of the module docstring asserted exactly, and no query
    redone (the precondition is asserted in grid_case, not assumed)"""
    gpu_or_skip()
    k = 10
    cb, codes, Q, want = grid_case(oracle, M, k)
    enc = _encoder(cb, codes)
    assert enc.ntotal == N_GRID and N_GRID % 64 != 0
    for nq in (1, 2, 3, 4, 5, 6, 7):
        lab, dist = enc.Search(Q[:nq], k)
        stats = enc.last_search_stats
        _assert_lists(lab, dist, want, (M, nq))
        assert stats == expected_stats(M, nq), (M, nq, stats)
    for i in range(7):
        l1, d1 = enc.Search(Q[i:i + 1], k)
        assert enc.last_search_stats == (1, 0, 0, 1, 0, 0), (M, i, enc.last_search_stats)
        assert np.array_equal(l1[0], lab[i]) and np.array_equal(d1[0], dist[i]), (M, i)
    enc.set_prefilter(False)
    l0, d0 = enc.Search(Q, k)
    assert enc.last_search_stats == expected_stats(M, 7, prefilter=False), (M, enc.last_search_stats)
    assert np.array_equal(l0, lab) and np.array_equal(d0, dist)
    enc.Close()


def test_m160_is_refused_and_m159_is_the_largest():
    gpu_or_skip()
    from longbow_amd import _lib
    with pytest.raises(_lib.LongbowGPUError) as e:
        _encoder(np.zeros((160, 256, 1), F))
    assert e.value.code == 6  # LB_ERR_UNSUPPORTED
    enc = _encoder(np.zeros((159, 256, 1), F))
    assert enc.M == 159
    enc.Close()


@pytest.mark.parametrize("M", [32, 48, 64, 128, 159])
def test_adc_distance_batch_forms(oracle, M):
    """ADCDistanceBatch over the whole corpus and over a window whose first row is not a multiple of 64: the DMA kernel
    at M = 32, 48, 64 (row_begin != 0), the staged 128 KiB table at M = 128 (no DMA form fits), the scalar kernel with
    the largest table LDS can hold at M = 159"""
    gpu_or_skip()
    rng = np.random.default_rng(500 + M)
    cb = rng.random((M, 256, 2), dtype=F)
    codes = rng.integers(0, 256, (N_GRID, M), dtype=np.uint8)
    enc = _encoder(cb, codes)
    q = rng.random(2 * M, dtype=F)
    table = enc.BuildADCTable(q)
    assert np.array_equal(table, oracle.build_adc_table(cb, q))
    want = oracle.adc_batch(table, codes)
    res = np.full(N_GRID, -1, F)
    enc.ADCDistanceBatch(table, res)
    assert np.array_equal(res, want)
    for row0, cnt in ((1237, 5000), (63, 4096), (N_GRID - 4097, 4097)):
        assert row0 % 64 != 0 and cnt >= 4096
        part = np.full(cnt, -1, F)
        enc.ADCDistanceBatch(table, part, row0=row0)
        assert np.array_equal(part, want[row0:row0 + cnt]), (M, row0)
    enc.Close()


# ---- planner edges ----------------------------------------------------------------------------------------------
def _check_search(oracle, enc, cb, codes, Q, k, ctx):
    """oracle equality, the plan the handle's counter reports, and no redone query.  For a sampled plan "no redo" is
    earned as in grid_case: on the oracle's distances the sampled tau admits between k rows and the list's capacity and
    the byte bound's survivors fit the candidate buffer -- asserted, then required of the device."""
    n, M = codes.shape
    assert enc.ntotal == n
    lab, dist = enc.Search(Q, k)
    stats = enc.last_search_stats
    want = _oracle_lists(oracle, cb, Q, codes, k)
    _assert_lists(lab, dist, want, ctx)
    cnt, m, _, cap = ab.plan(n, k)
    sampled = cnt != 0
    print(f"planner edge {ctx}: n={n} k={k} sampled={sampled} last_search_stats {stats}")
    assert stats[0] == (len(Q) if sampled else 0), (ctx, stats)
    if sampled:
        for b, (_, _, d, table) in enumerate(want):
            tau = ab.sampled_tau(d, cnt, m)
            admitted = int((d <= tau).sum())
            assert k <= admitted <= cap, (ctx, b, admitted)
            qt, s_tau, ok = ab.quantise(table.reshape(M, 256), tau)
            assert ok == 1 and int((ab.byte_sums(qt, codes) <= s_tau).sum()) <= ab.CAND_CAP, (ctx, b)
        assert stats[4] == 0 and stats[5] == 0, (ctx, stats)
    else:
        assert stats[1:5] == (0, 0, 0, 0), (ctx, stats)  # no sampled pass: nothing to miss, nothing redone on the bootstrap schedule
    return sampled, stats


def test_sampled_plan_starts_at_65536_rows(oracle):
    gpu_or_skip()
    rng = np.random.default_rng(65536)
    M = 16
    cb = rng.random((M, 256, 2), dtype=F)
    codes = rng.integers(0, 256, (65537, M), dtype=np.uint8)
    Q = rng.random((2, 2 * M), dtype=F)
    enc = _encoder(cb, codes[:65535])
    seen = {}
    for n in (65535, 65536, 65537):
        if n > 65535:
            enc.add_codes(codes[n - 1:n])
        seen[n] = _check_search(oracle, enc, cb, codes[:n], Q, 10, n)[0]
    assert seen == {65535: False, 65536: True, 65537: True}
    enc.Close()


def test_stride_switch_and_k_up_to_4096(oracle):
    """4,194,303 rows sample one row in 256, 4,194,304 one in 512; k = 1, 1000 and the supported maximum 4096 at both.
    Sampled (recorded from the planner's arithmetic, asserted on the handle's counter): k = 1 at both sizes, k = 1000 at
    4,194,303 rows only (one row in 512 would admit more than the list holds beside k), k = 4096 never (m > 32)."""
    gpu_or_skip()
    rng = np.random.default_rng(4194304)
    M, n1 = 16, 4194304
    cb = rng.random((M, 256, 2), dtype=F)
    codes = rng.integers(0, 256, (n1, M), dtype=np.uint8)
    Q = rng.random((2, 2 * M), dtype=F)
    assert ab.plan(n1 - 1, 1)[2] == 256 and ab.plan(n1, 1)[2] == 512
    enc = _encoder(cb, codes[:n1 - 1])
    seen = {}
    for n in (n1 - 1, n1):
        if n == n1:
            enc.add_codes(codes[n1 - 1:])
        for k in (1, 1000, 4096):
            seen[(n, k)] = _check_search(oracle, enc, cb, codes[:n], Q, k, (n, k))[0]
    assert seen == {(n1 - 1, 1): True, (n1 - 1, 1000): True, (n1 - 1, 4096): False,
                    (n1, 1): True, (n1, 1000): False, (n1, 4096): False}
    enc.Close()


def test_k_limits_and_k_beyond_ntotal(oracle):
    gpu_or_skip()
    from longbow_amd import _lib
    rng = np.random.default_rng(4097)
    M = 16
    cb = rng.random((M, 256, 2), dtype=F)
    codes = rng.integers(0, 256, (300, M), dtype=np.uint8)
    Q = rng.random((2, 2 * M), dtype=F)
    enc = _encoder(cb, codes)
    with pytest.raises(_lib.LongbowGPUError) as e:
        enc.Search(Q, 4097)
    assert e.value.code == 6  # LB_ERR_UNSUPPORTED
    _check_search(oracle, enc, cb, codes, Q, 10, "after the refusal")
    # k > ntotal: the ntotal rows in order, then label -1 / distance FLT_MAX (longbow_gpu.h: "fewer than k hits")
    lab, dist = enc.Search(Q, 1000)
    want = _oracle_lists(oracle, cb, Q, codes, 1000)
    for b in range(2):
        assert np.array_equal(lab[b, :300], want[b][0][:300]) and np.array_equal(dist[b, :300], want[b][1][:300])
        assert np.all(lab[b, 300:] == -1) and np.all(dist[b, 300:] == np.finfo(F).max)
    enc.Close()


def test_corpus_added_in_three_unequal_pieces(oracle):
    """the code buffer grows and is copied between the pieces; every size is searched (bootstrap, then sampled plans)"""
    gpu_or_skip()
    rng = np.random.default_rng(333)
    M = 48
    cb = rng.random((M, 256, 2), dtype=F)
    codes = rng.integers(0, 256, (70003, M), dtype=np.uint8)
    Q = rng.random((3, 2 * M), dtype=F)
    enc = _encoder(cb)
    for a, b in ((0, 5001), (5001, 66002), (66002, 70003)):
        enc.add_codes(codes[a:b])
        _check_search(oracle, enc, cb, codes[:b], Q, 10, b)
        assert np.array_equal(enc.get_codes(max(0, b - 100), min(100, b)), codes[max(0, b - 100):b])
    enc.Close()


# ---- table families ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [16, 96])
@pytest.mark.parametrize("name", ["dominant", "offset", "dyadic", "huge", "tiny"])
def test_table_families(oracle, name, M):
    """real codebooks and queries of each family (build_adc_table_kernel's min / range on the path), a quad and a single:
    oracle equality and prefilter on == off.  Redo counts may be non-zero (a dominant subtable overflows the candidate
    buffer, a tiny one is refused by the range floor); they are printed and carried in the failure message."""
    gpu_or_skip()
    rng = np.random.default_rng(7000 + M + len(name))
    k = 10
    cb, _ = family(name, M, 2, rng)
    Q = np.stack([family(name, M, 2, np.random.default_rng(7100 + i))[1] for i in range(5)])
    codes = rng.integers(0, 256, (N_GRID, M), dtype=np.uint8)
    enc = _encoder(cb, codes)
    want = _oracle_lists(oracle, cb, Q, codes, k)
    lab, dist = enc.Search(Q, k)
    stats = enc.last_search_stats
    print(f"table family {name} M={M}: last_search_stats {stats}")
    msg = (name, M, "stats", stats)
    assert stats[:4] == (5, 4, 0, 1), msg  # a quad in the four-query form and a single, at M = 16 and at M = 96
    for b in range(5):
        assert np.array_equal(lab[b], want[b][0]) and np.array_equal(dist[b], want[b][1]), msg + (b,)
    if name == "tiny":
        assert stats[4] == 5, msg  # below the range floor every query is refused and served by the exact schedule
    enc.set_prefilter(False)
    l0, d0 = enc.Search(Q, k)
    assert np.array_equal(l0, lab) and np.array_equal(d0, dist), msg
    enc.Close()


def test_tiny_magnitude_wrong_survivors(oracle):
    """the corpus of tests/test_adc_bound_semantics.py on which a byte bound with 255 / rmax = +inf keeps at least k
    WRONG rows (so no redo would repair it): the device must return the oracle's list, by refusing the prefilter
    (the query is redone on the exact schedule)"""
    gpu_or_skip()
    k = 10
    cb, q, codes, near = wrong_survivor_corpus(N_GRID)
    enc = _encoder(cb, codes)
    want = _oracle_lists(oracle, cb, q[None], codes, k)
    assert set(want[0][0][:5]) == set(near)
    lab, dist = enc.Search(q, k)
    stats = enc.last_search_stats
    print(f"tiny-magnitude wrong survivors: last_search_stats {stats}")
    assert np.array_equal(lab[0], want[0][0]) and np.array_equal(dist[0], want[0][1]), (stats, lab[0], want[0][0])
    assert stats == (1, 0, 0, 1, 1, 0), stats
    enc.Close()


@pytest.mark.parametrize("M", [16, 96])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_query_in_each_position_of_a_quad(oracle, bad, M):
    """adc_prefilter4_kernel<1, 16> and <6, 10> (the config-4 shape) with one query of the four refused on the device"""
    gpu_or_skip()
    rng = np.random.default_rng(44 + M)
    k = 10
    cb = rng.random((M, 256, 2), dtype=F)
    codes = rng.integers(0, 256, (N_GRID, M), dtype=np.uint8)
    Q = rng.random((4, 2 * M), dtype=F)
    enc = _encoder(cb, codes)
    for pos in range(4):
        Qb = Q.copy()
        Qb[pos, 5] = bad
        lab, dist = enc.Search(Qb, k)
        stats = enc.last_search_stats
        assert stats[:4] == (4, 4, 0, 0) and stats[4] >= 1, (M, pos, stats)  # the quad ran; the bad query was redone exactly
        _assert_lists(lab, dist, _oracle_lists(oracle, cb, Qb, codes, k), (bad, M, pos, stats))
    enc.Close()


# ---- codec ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [2, 16, 32, 24, 3])
def test_encode_sub_dimensions_and_block_edges(oracle, sub):
    """SubDim 2, 16, 32 (templated kernels) and 24, 3 (generic kernel); 1, 255, 256, 257 rows around the 256-row block"""
    gpu_or_skip()
    rng = np.random.default_rng(600 + sub)
    M = 3
    cb = rng.random((M, 256, sub), dtype=F)
    enc = _encoder(cb)
    V = rng.random((257, M * sub), dtype=F)
    want = np.stack([oracle.pq_encode(cb, v) for v in V])
    for n in (1, 255, 256, 257):
        assert np.array_equal(enc.Encode(V[:n]), want[:n]), (sub, n)
    enc.Close()


@pytest.mark.parametrize("sub", [4, 3])
@pytest.mark.parametrize("nan_centroid", [None, 0, 7])
def test_encode_non_finite_inputs(oracle, sub, nan_centroid):
    """NaN, +Inf and -Inf in one sub-vector, and a NaN centroid at index 0 or 7: the reference's strict `<` keeps
    index 0 whenever every comparison is false (templated SubDim 4 and the generic kernel at SubDim 3)"""
    gpu_or_skip()
    rng = np.random.default_rng(800 + sub)
    M = 4
    cb = rng.random((M, 256, sub), dtype=F)
    if nan_centroid is not None:
        cb[1, nan_centroid, sub - 1] = np.nan
    enc = _encoder(cb)
    V = rng.random((64, M * sub), dtype=F)
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):
        for m in range(M):
            V[4 * i + m, m * sub + (m % sub)] = bad
    V[20, sub:2 * sub] = (np.nan, np.inf, -np.inf, 1.0)[:sub]
    want = np.stack([oracle.pq_encode(cb, v) for v in V])
    got = enc.Encode(V)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert got[0, 0] == 0 and got[4, 0] == 0 and got[8, 0] == 0  # a non-finite sub-vector keeps centroid 0
    enc.Close()


def test_decode_grid_stride_loop_and_single_row(oracle):
    """6,000 rows x 768 dimensions = 4.6M elements: more than the 16,384 x 256 threads of the launch, so the loop wraps"""
    gpu_or_skip()
    rng = np.random.default_rng(768)
    M, sub, n = 96, 8, 6000
    assert n * M * sub > 16384 * 256
    cb = rng.random((M, 256, sub), dtype=F)
    enc = _encoder(cb)
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    dec = enc.Decode(codes)
    want = np.stack([oracle.pq_decode(cb, c) for c in codes])
    assert np.array_equal(dec, want)
    assert np.array_equal(enc.Decode(codes[5999]), want[5999])
    assert np.array_equal(enc.Decode(codes[:1]), want[:1])
    enc.Close()
