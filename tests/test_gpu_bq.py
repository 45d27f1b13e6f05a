"""lb_gpu_bq_* on the GPU against tests/bq_oracle.py.  Every comparison is exact: codes, integer distances, labels."""
import numpy as np
import pytest

from tests import bq_oracle as bo
from tests.gpu_util import gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(F).max


def _enc(dims):
    gpu_or_skip()
    from longbow_amd import bq
    return bq.BQEncoder(dims)


def _rand_codes(rng, n, dims):
    """uniform random bits, pad bits zero"""
    W = bo.words(dims)
    c = rng.integers(0, 1 << 64, (n, W), dtype=np.uint64)
    if dims % 64:
        c[:, -1] &= np.uint64((1 << (dims % 64)) - 1)
    return c


def _special_rows(dims):
    tiny = F(1e-45)
    vals = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, tiny, -tiny, np.finfo(F).tiny, -np.finfo(F).tiny, 1.0, -1.0], F)
    return np.stack([np.resize(np.roll(vals, s), dims) for s in range(vals.size)])


# ---- codec ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("dims", [1, 63, 64, 65, 100, 768, 1000, 8192])
def test_codec_matches_the_oracle(dims, n):
    enc = _enc(dims)
    rng = np.random.default_rng(dims * 7 + n)
    X = (rng.random((n, dims), dtype=F) - F(0.5)).astype(F)
    X[rng.random((n, dims)) < 0.05] = 0.0
    want = bo.encode(X)
    assert enc.CodeSize() == bo.words(dims) == want.shape[1]
    codes = enc.Encode(X)
    assert codes.dtype == np.uint64 and np.array_equal(codes, want)
    assert np.array_equal(enc.Encode(X[0]), want[0])
    assert np.array_equal(enc.Decode(codes), np.where(X > 0, F(1), F(-1)))
    assert np.array_equal(enc.Decode(codes), bo.decode(want, dims))
    enc.add_vectors(X)
    assert enc.ntotal == n and np.array_equal(enc.get_codes(), want)
    enc.Close()


@pytest.mark.parametrize("dims", [12, 100, 768])
def test_codec_special_values(dims):
    enc = _enc(dims)
    X = _special_rows(dims)
    want = bo.encode(X)
    assert np.array_equal(enc.Encode(X), want)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(enc.Decode(want), np.where(X > 0, F(1), F(-1)))
    enc.add_vectors(X)
    assert np.array_equal(enc.get_codes(), want)
    enc.Close()


def test_device_pointer_codec_and_adds_equal_the_host_forms():
    import torch
    dims, n = 100, 777
    enc = _enc(dims)
    rng = np.random.default_rng(3)
    X = (rng.random((n, dims), dtype=F) - F(0.5)).astype(F)
    want = bo.encode(X)
    dX = torch.from_numpy(X).cuda()
    dC = torch.zeros((n, enc.W), dtype=torch.int64, device="cuda")
    enc.encode_device(n, dX.data_ptr(), dC.data_ptr())
    assert np.array_equal(dC.cpu().numpy().view(np.uint64), want)
    enc.add_vectors_device(n, dX.data_ptr())
    enc.add_codes_device(n, dC.data_ptr())
    enc.add_vectors(X[:5])
    enc.add_codes(want[:3])
    assert enc.ntotal == 2 * n + 8
    assert np.array_equal(enc.get_codes(), np.concatenate([want, want, want[:5], want[:3]]))
    assert np.array_equal(enc.get_codes(n - 1, 3), np.concatenate([want[-1:], want[:2]]))
    enc.Close()


# ---- golden -----------------------------------------------------------------------------------------------------------------
def test_golden_cases_through_the_library():
    kenc, kham = bo.load_kats()
    for name, v, codes in kenc:
        enc = _enc(v.size)
        assert np.array_equal(enc.Encode(v), codes), name
        enc.Close()
    for name, a, b, expected in kham:
        if a.size == 0:
            continue  # (a handle has at least one word: the empty case is the oracle's alone)
        enc = _enc(64 * a.size)
        enc.add_codes(b.reshape(1, -1))
        assert enc.HammingDistanceBatch(a).tolist() == [expected], name
        assert enc.HammingDistance(a, b) == expected, name
        enc.Close()


def test_pad_bits_of_added_codes_count():
    dims = 100
    enc = _enc(dims)
    rng = np.random.default_rng(11)
    codes = rng.integers(0, 1 << 64, (300, 2), dtype=np.uint64)  # bits 100..127 set at random
    q = rng.integers(0, 1 << 64, 2, dtype=np.uint64)
    codes[7] = ~q  # all 128 bits differ: a distance above dims
    enc.add_codes(codes)
    assert np.array_equal(enc.get_codes(), codes)
    want = bo.hamming(q, codes)
    assert want.max() == 128 > dims
    assert np.array_equal(enc.HammingDistanceBatch(q), want)
    lab, dist = enc.search_codes(q, 300)
    olab, odist = bo.topk(want, 300)
    assert np.array_equal(lab[0], olab) and np.array_equal(dist[0], odist)
    enc.Close()


# ---- hamming_batch / rerank -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [64, 768, 8192])
def test_hamming_batch_and_rerank(dims):
    n = 3001
    enc = _enc(dims)
    rng = np.random.default_rng(dims)
    codes = _rand_codes(rng, n, dims)
    q = _rand_codes(rng, 1, dims)[0]
    enc.add_codes(codes)
    want = bo.hamming(q, codes)
    got = enc.HammingDistanceBatch(q)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(enc.HammingDistanceBatch(q, row0=100, n=700), want[100:800])  # starts and ends inside a tile
    assert np.array_equal(enc.HammingDistanceBatch(q, row0=3000, n=1), want[3000:])
    assert enc.HammingDistanceBatch(q, row0=5, n=0).size == 0
    assert np.array_equal(enc.HammingDistanceBatch(q, codes[:300]), want[:300])
    rows = np.concatenate([rng.integers(0, n, 600), [-1, n, 0, 0, n - 1, 2**40, -(2**40)]]).astype(np.int64)
    ok = (rows >= 0) & (rows < n)
    wd = np.where(ok, want[np.clip(rows, 0, n - 1)].astype(F), FLT_MAX).astype(F)
    ws = np.where(ok, bo.score(want[np.clip(rows, 0, n - 1)], dims), F(0)).astype(F)
    dist, score = enc.rerank(q, rows)
    assert np.array_equal(dist, wd) and np.array_equal(score, ws)
    assert np.array_equal(enc.rerank(q, rows, want_score=False), wd)  # a null score
    assert np.array_equal(enc.ScoreToFloat32(want[:50]), bo.score(want[:50], dims))
    from longbow_amd import _lib
    with pytest.raises(_lib.LongbowGPUError):
        enc.HammingDistanceBatch(q, row0=n - 1, n=2)
    enc.Close()


def test_rerank_on_an_empty_handle_and_device_form():
    import torch
    enc = _enc(768)
    q = _rand_codes(np.random.default_rng(1), 1, 768)[0]
    d, s = enc.rerank(q, [0, 5])
    assert np.all(d == FLT_MAX) and np.all(s == 0)
    codes = _rand_codes(np.random.default_rng(2), 500, 768)
    enc.add_codes(codes)
    rows = np.array([3, 499, 500, 3, -1], np.int64)
    dq = torch.from_numpy(q.view(np.int64)).cuda()
    dr = torch.from_numpy(rows).cuda()
    dd = torch.zeros(5, dtype=torch.float32, device="cuda")
    ds = torch.zeros(5, dtype=torch.float32, device="cuda")
    enc.rerank_device(dq.data_ptr(), dr.data_ptr(), 5, dd.data_ptr(), ds.data_ptr())
    hd, hs = enc.rerank(q, rows)
    assert np.array_equal(dd.cpu().numpy(), hd) and np.array_equal(ds.cpu().numpy(), hs)
    assert hd[2] == FLT_MAX and hd[4] == FLT_MAX and hd[0] == hd[3] == F(bo.hamming(q, codes[3:4])[0])
    enc.Close()


# ---- search against the oracle ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def search_case():
    """search_case(key, make) -> (index, query codes, oracle labels, oracle distances at k = min(2048, n), whose prefixes are the
    smaller k): make(rng) -> (codes, qcodes) runs once per key; the handles are closed and the arrays dropped with the module"""
    cache = {}

    def get(key, make):
        if key not in cache:
            dims, n = key[0], key[1]
            codes, qcodes = make(np.random.default_rng(dims + n))
            assert codes.shape == (n, bo.words(dims))
            enc = _enc(dims)
            enc.add_codes(codes)
            cache[key] = (enc, qcodes) + bo.search(qcodes, codes, min(2048, n))
        return cache[key]

    yield get
    for case in cache.values():
        case[0].Close()
    cache.clear()


def _random_case(dims, n, nq):
    return lambda rng: (_rand_codes(rng, n, dims), _rand_codes(rng, nq, dims))


@pytest.mark.parametrize("k", [1, 100, 2048])
@pytest.mark.parametrize("nq", [1, 2, 7, 33, 257])
@pytest.mark.parametrize("dims", [65, 768, 1000])
def test_search_matches_the_oracle(search_case, dims, nq, k):
    enc, qcodes, olab, odist = search_case((dims, 70001), _random_case(dims, 70001, 257))
    lab, dist = enc.search_codes(qcodes[:nq], k)
    assert lab.shape == (nq, k) and dist.dtype == F
    assert np.array_equal(lab, olab[:nq, :k]), np.argwhere(lab != olab[:nq, :k])[:5]
    assert np.array_equal(dist, odist[:nq, :k])


def test_search_widest_rows(search_case):
    enc, qcodes, olab, odist = search_case((8192, 5000), _random_case(8192, 5000, 3))
    lab, dist = enc.search_codes(qcodes, 10)
    assert np.array_equal(lab, olab[:, :10]) and np.array_equal(dist, odist[:, :10])


def test_search_mid_size():
    n, dims, nq, k = 200000, 768, 64, 100
    rng = np.random.default_rng(2024)
    codes = _rand_codes(rng, n, dims)
    qcodes = _rand_codes(rng, nq, dims)
    enc = _enc(dims)
    enc.add_codes(codes)
    lab, dist = enc.search_codes(qcodes, k)
    olab, odist = bo.search(qcodes, codes, k)
    assert np.array_equal(lab, olab) and np.array_equal(dist, odist)
    enc.Close()


# ---- several tiles per workgroup, several batches of queries ----------------------------------------------------------------
# A search runs at most 2048 workgroups, each over a contiguous run of whole 256-row tiles: beyond 2048 * 256 = 524,288 rows a
# workgroup walks more than one tile, carrying its LDS histogram, its counts and its emit offsets from tile to tile.  Every
# index of the size this handle is for (1M rows: two tiles, 10M: twenty) searches that way.  600,257 rows are 2,345 tiles: 1,172
# workgroups of two tiles, a last one of a single tile, of 193 rows.  One word per row keeps it at 4.8 MB.
_TWO_TILE_N = 600257
assert 2048 < -(-_TWO_TILE_N // 256) < 2 * 2048 and -(-_TWO_TILE_N // 256) % 2 == 1 and _TWO_TILE_N % 256


def _tie_case(rng):
    """Three codes A, B, C at distances d(A,B) = 3, d(A,C) = 10, d(B,C) = 13.  A: about one row in 2048, in every tile.  B: about
    every other row of the odd tiles (each workgroup's second) and nowhere else.  C: the rest, so nearly all of the even tiles.
    With the queries A, B, C themselves, rows below the threshold lie in both tiles of a workgroup, and the k-th row (where
    `need` runs out) lies in a workgroup's second tile for B (k = 100: tile 1; k = 2048: tile 31 or so) and for A at k = 2048
    (about 293 rows of A below t, then 1,755 of B); for C the ties span both tiles of the first workgroups."""
    n = _TWO_TILE_N
    a = _rand_codes(rng, 1, 64)[0, 0]
    three = np.array([[a], [a ^ np.uint64(0b111)], [a ^ np.uint64(0x3FF << 20)]], np.uint64)
    tile = np.arange(n) // 256
    which = np.where((tile % 2 == 1) & (rng.random(n) < 0.5), 1, 2)
    which[rng.random(n) < 1 / 2048] = 0
    assert 100 < (which == 0).sum() < 2048 and (which[:256] == 1).sum() == 0 and 100 < (which[256:512] == 1).sum()
    return three[which].reshape(n, 1), np.concatenate([three, _rand_codes(rng, 4, 64)])


@pytest.mark.parametrize("k", [100, 2048])
@pytest.mark.parametrize("first,nq", [(0, 1), (1, 1), (2, 1), (0, 7)])
@pytest.mark.parametrize("corpus", ["random", "ties"])
def test_search_two_tiles_per_workgroup(search_case, corpus, first, nq, k):
    make = _tie_case if corpus == "ties" else _random_case(64, _TWO_TILE_N, 7)
    enc, qcodes, olab, odist = search_case((64, _TWO_TILE_N, corpus), make)
    sel = slice(first, first + nq)
    lab, dist = enc.search_codes(qcodes[sel], k)
    assert np.array_equal(lab, olab[sel, :k]), np.argwhere(lab != olab[sel, :k])[:5]
    assert np.array_equal(dist, odist[sel, :k])


# The scan of the per-workgroup counts (countsel_scan_kernel, shared with the SQ8 index) gives each of its 256 threads
# ceil(nblk / 256) workgroups.  70,145 rows are 275 tiles, one workgroup each: two per thread, and the last occupied thread owns
# the single workgroup 274, whose tile holds one row.
_SCAN_N = 70145
assert -(-_SCAN_N // 256) == 275 and _SCAN_N % 256 == 1


def _three_values_case(rng):
    """Three distinct codes assigned at random, the last row among the first's: with the three as queries the rows at the
    threshold (distance 0) lie in nearly every workgroup, and the last one is the last row of the corpus.  A fourth code on
    about one row in 70 and as the fourth query: at k = 2048 its thousand rows are the rows BELOW the threshold, a few in most
    workgroups, so the scan of both counts is pinned."""
    four = _rand_codes(rng, 4, 64)
    assert np.unique(four).size == 4
    which = rng.integers(0, 3, _SCAN_N)
    which[rng.random(_SCAN_N) < 1 / 70] = 3
    which[-1] = 0
    assert 100 < (which == 3).sum() < 2048 and np.unique(np.flatnonzero(which == 3) // 256).size > 200
    return four[which], four


@pytest.mark.parametrize("k", [100, 2048])
def test_search_scan_gives_a_thread_two_workgroups(search_case, k):
    enc, qcodes, olab, odist = search_case((64, _SCAN_N, "three values"), _three_values_case)
    lab, dist = enc.search_codes(qcodes, k)
    assert np.array_equal(lab, olab[:, :k]), np.argwhere(lab != olab[:, :k])[:5]
    assert np.array_equal(dist, odist[:, :k])


@pytest.mark.parametrize("nq", [1025, 2049])
def test_search_more_queries_than_one_batch(nq):
    """the selection runs 1024 queries at a time over one scratch: the second and third batch reuse the histograms, counts and
    keys of the first, and read their queries and write their results at an offset"""
    dims, n, k = 100, 3001, 37
    rng = np.random.default_rng(nq)
    codes = _rand_codes(rng, n, dims)
    qcodes = _rand_codes(rng, nq, dims)
    enc = _enc(dims)
    enc.add_codes(codes)
    lab, dist = enc.search_codes(qcodes, k)
    enc.Close()
    d = sum(np.bitwise_count(qcodes[:, None, w] ^ codes[None, :, w]).astype(np.int32) for w in range(codes.shape[1]))  # [nq, n]
    olab = np.argsort(d, axis=1, kind="stable")[:, :k]  # stable: the lowest position wins a tie, as bo.topk's lexsort
    assert np.array_equal(olab[:3], bo.search(qcodes[:3], codes, k)[0])
    assert np.array_equal(lab, olab), np.argwhere(lab != olab)[:5]
    assert np.array_equal(dist, np.take_along_axis(d, olab, axis=1).astype(F))


# ---- ties -------------------------------------------------------------------------------------------------------------------
def test_identical_rows():
    dims = 768
    enc = _enc(dims)
    rng = np.random.default_rng(5)
    code = _rand_codes(rng, 1, dims)
    q = _rand_codes(rng, 2, dims)
    q[1] = code[0]
    enc.add_codes(np.repeat(code, 5000, axis=0))
    lab, dist = enc.search_codes(q, 100)
    for i in range(2):
        assert lab[i].tolist() == list(range(100))
        assert np.all(dist[i] == F(bo.hamming(q[i], code)[0]))
    lab, dist = enc.search_codes(q, 2048)
    assert lab[0].tolist() == list(range(2048)) and lab[1].tolist() == list(range(2048)) and np.all(dist[1] == 0)
    enc.Close()


@pytest.mark.parametrize("dims", [100, 768])
def test_interleaved_ties_and_k_around_the_threshold(dims):
    n = 5000
    enc = _enc(dims)
    rng = np.random.default_rng(dims)
    three = _rand_codes(rng, 3, dims)
    which = np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 7 == 0, 2, 1))  # interleaved through every workgroup
    codes = three[which]
    enc.add_codes(codes)
    q = three[:1]
    d = bo.hamming(q[0], codes)
    n0 = int((which == 0).sum())
    below = int((d <= np.sort(np.unique(d))[1]).sum())  # rows at the two nearest distances
    assert n0 < 2048
    ks = [n0 - 1, n0, n0 + 1, n0 + 300, 1, 2048] + ([below - 1, below, below + 1] if below + 1 <= 2048 else [])
    for k in ks:
        lab, dist = enc.search_codes(q, k)
        olab, odist = bo.topk(d, k)
        assert np.array_equal(lab[0], olab), k
        assert np.array_equal(dist[0], odist), k
    # several queries at once, each with its own threshold
    lab, dist = enc.search_codes(three, n0 + 37)
    olab, odist = bo.search(three, codes, n0 + 37)
    assert np.array_equal(lab, olab) and np.array_equal(dist, odist)
    enc.Close()


# ---- small n, growth --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_small_n_pads(n):
    dims = 130
    enc = _enc(dims)
    rng = np.random.default_rng(n)
    codes = _rand_codes(rng, n, dims)
    q = _rand_codes(rng, 3, dims)
    if n:
        enc.add_codes(codes)
    for k in sorted({n + 1, n + 40, max(n, 1), 1}):
        lab, dist = enc.search_codes(q, k)
        olab, odist = bo.search(q, codes, k)
        assert np.array_equal(lab, olab), (n, k)
        assert np.array_equal(dist, odist), (n, k)
    enc.Close()


def test_growth_keeps_positions():
    dims = 768
    enc = _enc(dims)
    rng = np.random.default_rng(8)
    codes = _rand_codes(rng, 100 + 5000 + 3000, dims)
    q = _rand_codes(rng, 4, dims)
    at = 0
    for cnt in (100, 5000, 3000):  # no reserve: the second and third add re-allocate
        enc.add_codes(codes[at:at + cnt])
        at += cnt
        assert enc.ntotal == at
        lab, dist = enc.search_codes(q, 50)
        olab, odist = bo.search(q, codes[:at], 50)
        assert np.array_equal(lab, olab) and np.array_equal(dist, odist)
    assert np.array_equal(enc.get_codes(), codes)
    enc.reserve(20000)
    assert enc.ntotal == at and np.array_equal(enc.get_codes(90, 20), codes[90:110])
    enc.Close()


# ---- f32 entry points, limits, cancellation ---------------------------------------------------------------------------------
def test_f32_search_entry_points_and_limits():
    import torch
    from longbow_amd import _lib, gpu
    dims, n, nq, k = 100, 4000, 5, 20
    enc = _enc(dims)
    rng = np.random.default_rng(21)
    X = (rng.random((n, dims), dtype=F) - F(0.5)).astype(F)
    Q = (rng.random((nq, dims), dtype=F) - F(0.5)).astype(F)
    enc.add_vectors(X)
    lab, dist = enc.search(Q, k)
    clab, cdist = enc.search_codes(enc.Encode(Q), k)
    olab, odist = bo.search(bo.encode(Q), bo.encode(X), k)
    assert np.array_equal(lab, clab) and np.array_equal(dist, cdist)
    assert np.array_equal(lab, olab) and np.array_equal(dist, odist)
    dQ = torch.from_numpy(Q).cuda()
    dD = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    dL = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    enc.search_device(nq, dQ.data_ptr(), k, dD.data_ptr(), dL.data_ptr())
    assert np.array_equal(dL.cpu().numpy(), lab) and np.array_equal(dD.cpu().numpy(), dist)
    # a fired context: nothing is launched, nothing is written
    ctx = gpu.Cancel()
    ctx.fire()
    with pytest.raises(_lib.Canceled):
        enc.search(Q, k, ctx=ctx)
    dD.fill_(-5.0)
    with pytest.raises(_lib.Canceled):
        enc.search_device(nq, dQ.data_ptr(), k, dD.data_ptr(), dL.data_ptr(), ctx=ctx)
    torch.cuda.synchronize()
    assert bool((dD == -5.0).all())
    ctx.close()
    live = gpu.Cancel()
    lab2, dist2 = enc.search(Q, k, ctx=live)  # a context that never fires changes nothing
    assert np.array_equal(lab2, lab) and np.array_equal(dist2, dist)
    live.close()
    # behind a live handle: INVALID_ARG before UNSUPPORTED, and a refused call writes nothing
    lib, h = enc._lib, enc._h
    d = np.full(nq * 3000, 9.0, F)
    l = np.full(nq * 3000, 77, np.int64)
    q = np.ascontiguousarray(Q)
    assert lib.lb_gpu_bq_search(h, nq, q.ctypes.data, 0, d.ctypes.data, l.ctypes.data) == 1
    assert lib.lb_gpu_bq_search(h, nq, q.ctypes.data, -3, d.ctypes.data, l.ctypes.data) == 1
    assert lib.lb_gpu_bq_search(h, -1, q.ctypes.data, 2049, d.ctypes.data, l.ctypes.data) == 1
    assert lib.lb_gpu_bq_search(h, nq, None, 2049, d.ctypes.data, l.ctypes.data) == 1
    assert lib.lb_gpu_bq_search(h, nq, q.ctypes.data, 2049, d.ctypes.data, l.ctypes.data) == 6
    assert lib.lb_gpu_bq_search_codes(h, nq, q.ctypes.data, 2049, d.ctypes.data, l.ctypes.data) == 6
    assert b"2049" in lib.lb_gpu_bq_last_error(h)
    assert lib.lb_gpu_bq_search(h, 0, None, 5, None, None) == 0
    assert lib.lb_gpu_bq_get_codes(h, n - 1, 2, d.ctypes.data) == 1
    assert lib.lb_gpu_bq_reserve(h, 1 << 31) == 6
    # a negative n, a negative row and a null pointer, behind a live handle: INVALID_ARG from every entry point
    c = np.full(8, 0xABABABABABABABAB, np.uint64)
    v = np.full(4 * dims, 7.0, F)
    r = np.arange(4, dtype=np.int64)
    o = np.full(4, 0x5A5A5A5A, np.int32)
    cp, vp, rp, op, dp = c.ctypes.data, v.ctypes.data, r.ctypes.data, o.ctypes.data, d.ctypes.data
    refused = [
        lib.lb_gpu_bq_add_codes(h, -1, cp), lib.lb_gpu_bq_add_codes(h, 1, None),
        lib.lb_gpu_bq_add_codes_device(h, -1, cp), lib.lb_gpu_bq_add_codes_device(h, 1, None),
        lib.lb_gpu_bq_add_vectors(h, -1, vp), lib.lb_gpu_bq_add_vectors(h, 1, None),
        lib.lb_gpu_bq_add_vectors_device(h, -1, vp), lib.lb_gpu_bq_add_vectors_device(h, 1, None),
        lib.lb_gpu_bq_encode(h, -1, vp, cp), lib.lb_gpu_bq_encode(h, 1, None, cp), lib.lb_gpu_bq_encode(h, 1, vp, None),
        lib.lb_gpu_bq_encode_device(h, -1, vp, cp, None), lib.lb_gpu_bq_encode_device(h, 1, None, cp, None),
        lib.lb_gpu_bq_encode_device(h, 1, vp, None, None),
        lib.lb_gpu_bq_decode(h, -1, cp, vp), lib.lb_gpu_bq_decode(h, 1, None, vp), lib.lb_gpu_bq_decode(h, 1, cp, None),
        lib.lb_gpu_bq_hamming_batch(h, cp, 0, -1, op), lib.lb_gpu_bq_hamming_batch(h, cp, -1, 1, op),
        lib.lb_gpu_bq_hamming_batch(h, None, 0, 1, op), lib.lb_gpu_bq_hamming_batch(h, cp, 0, 1, None),
        lib.lb_gpu_bq_rerank(h, cp, rp, -1, dp, None), lib.lb_gpu_bq_rerank(h, None, rp, 1, dp, None),
        lib.lb_gpu_bq_rerank(h, cp, None, 1, dp, None), lib.lb_gpu_bq_rerank(h, cp, rp, 1, None, None),
        lib.lb_gpu_bq_rerank_device(h, cp, rp, -1, dp, None, None), lib.lb_gpu_bq_rerank_device(h, None, rp, 1, dp, None, None),
        lib.lb_gpu_bq_rerank_device(h, cp, None, 1, dp, None, None), lib.lb_gpu_bq_rerank_device(h, cp, rp, 1, None, None, None),
        lib.lb_gpu_bq_get_codes(h, 0, -1, cp), lib.lb_gpu_bq_get_codes(h, -1, 1, cp), lib.lb_gpu_bq_get_codes(h, 0, 1, None),
        lib.lb_gpu_bq_reserve(h, -1),
    ]
    assert refused == [1] * len(refused), refused
    assert lib.lb_gpu_bq_ntotal(h) == n and np.array_equal(enc.get_codes(), bo.encode(X))
    assert (c == 0xABABABABABABABAB).all() and (v == 7.0).all() and (o == 0x5A5A5A5A).all() and (r == np.arange(4)).all()
    assert (d == 9.0).all() and (l == 77).all()
    assert lib.lb_gpu_bq_dims(h) == dims and lib.lb_gpu_bq_words(h) == 2
    lab, dist = enc.search(Q, 2048)  # k = LB_MAX_K is served
    assert np.array_equal(lab, bo.search(bo.encode(Q), bo.encode(X), 2048)[0])
    enc.Close()


def test_search_rerank_composition(oracle):
    from longbow_amd import bq
    n, dims, nq, k, over = 20000, 128, 4, 10, 10
    rng = np.random.default_rng(77)
    X = (rng.random((n, dims), dtype=F) - F(0.5)).astype(F)
    Q = (X[rng.integers(0, n, nq)] + F(0.05) * (rng.random((nq, dims), dtype=F) - F(0.5))).astype(F)
    enc = _enc(dims)
    enc.add_vectors(X)
    idx = new_index(dims, 0)
    idx.Add(None, X)
    lab, dist = bq.search_rerank(enc, idx, Q, k, over)
    short, _ = bo.search(bo.encode(Q), bo.encode(X), k * over)
    for i in range(nq):
        d = oracle.batch_flat(0, Q[i], X[short[i]], 1)
        keep = np.lexsort((short[i], d))[:k]
        assert np.array_equal(lab[i], short[i][keep]) and np.array_equal(dist[i], d[keep])
    assert np.array_equal(enc.search_rerank(idx, Q, k, over)[0], lab)
    idx.Close()
    enc.Close()
