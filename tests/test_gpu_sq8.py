"""lb_gpu_sq8_* on the GPU against tests/sq8_oracle.py.  Every comparison is exact: bounds, codes, decoded values, integer
distances, the decoded-space distance, labels."""
import numpy as np
import pytest

from tests import sq8_oracle as so
from tests.gpu_util import gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(F).max
INT32_MAX = 0x7FFFFFFF
TILE = 256
MAX_BLOCKS = 1024  # SQ8_MAX_BLOCKS (lb_device.h): the workgroups that share the rows of a search


def _enc(dims):
    gpu_or_skip()
    from longbow_amd import sq8
    return sq8.SQ8Encoder(dims)


def _same(a, b):
    """bit for bit up to the sign of a zero and the payload of a NaN"""
    return np.array_equal(a, b, equal_nan=True)


def _check_search(enc, Q, codes, ks, ctx=""):
    """search_codes against the oracle for each k, the oracle's order computed once per query"""
    S = np.stack([so.dist_s(q, codes) for q in Q]) if codes.shape[0] else np.zeros((Q.shape[0], 0), np.int32)
    order = [np.lexsort((np.arange(S.shape[1]), s)) for s in S]
    for k in ks:
        lab, dist = enc.search_codes(Q, k)
        for i in range(Q.shape[0]):
            o = order[i][:k]
            want_l = np.full(k, -1, np.int64)
            want_d = np.full(k, FLT_MAX, F)
            want_l[:o.size] = o
            want_d[:o.size] = S[i][o].astype(F)
            assert np.array_equal(lab[i], want_l), f"{ctx} k={k} query {i}: {np.argwhere(lab[i] != want_l)[:5].ravel()}"
            assert np.array_equal(dist[i], want_d), f"{ctx} k={k} query {i}"


# ---- codec and training -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("dims", [1, 3, 4, 15, 16, 17, 100, 768, 8192])
def test_training_and_codec_match_the_oracle(dims, n):
    rng = np.random.default_rng(dims * 7 + n)
    X = (rng.random((n, dims), dtype=F) * F(2) - F(1)).astype(F)
    Y = (rng.random((64, dims), dtype=F) * F(3) - F(1.5)).astype(F)  # beyond the bounds on both sides
    Y[0], Y[1] = X.min(axis=0), X.max(axis=0)                         # exactly on them
    mn, mx = so.train(X)
    enc = _enc(dims)
    assert not enc.trained and enc.Dims() == dims
    enc.train(X)
    assert enc.trained
    gmn, gmx = enc.GetBounds()
    assert np.array_equal(gmn, mn) and np.array_equal(gmx, mx)
    for V in (X, Y):
        want = so.encode(V, mn, mx)
        codes = enc.Encode(V)
        assert codes.dtype == np.uint8 and np.array_equal(codes, want)
        assert np.array_equal(enc.Decode(codes), so.decode(want, mn, mx))
    assert np.array_equal(enc.Encode(Y[3]), so.encode(Y[3], mn, mx))
    allc = np.arange(256, dtype=np.uint8).repeat(dims).reshape(256, dims)
    assert np.array_equal(enc.Decode(allc), so.decode(allc, mn, mx))
    enc.add_vectors(Y)
    assert enc.ntotal == 64 and np.array_equal(enc.get_codes(), so.encode(Y, mn, mx))
    # set_bounds on the same bounds is the same encoder
    enc2 = _enc(dims)
    enc2.set_bounds(mn, mx)
    assert np.array_equal(enc2.Encode(Y), so.encode(Y, mn, mx))
    b2 = enc2.GetBounds()
    assert np.array_equal(b2[0], mn) and np.array_equal(b2[1], mx)
    enc.Close()
    enc2.Close()


def test_training_is_the_same_from_run_to_run_and_for_the_device_pointer():
    import torch
    gpu_or_skip()
    dims, n = 100, 5000
    rng = np.random.default_rng(2)
    X = rng.standard_normal((n, dims)).astype(F)
    X[rng.random((n, dims)) < 0.01] = np.nan
    X[0] = rng.standard_normal(dims).astype(F)
    mn, mx = so.train(X)
    dX = torch.from_numpy(X).cuda()
    for rep in range(3):
        enc = _enc(dims)
        if rep == 2:
            enc.train_device(n, dX.data_ptr())
        else:
            enc.train(X)
        b = enc.GetBounds()
        assert b[0].tobytes() == mn.tobytes() and b[1].tobytes() == mx.tobytes()
        enc.Close()


def test_training_special_cases():
    from longbow_amd import _lib, sq8
    nan = F(np.nan)
    # a NaN in row 0 stays, a NaN in a later row is ignored; NaN bounds pass Validate
    X = np.array([[nan, 1.0, 3.0], [2.0, nan, 1.0], [5.0, 4.0, nan], [-1.0, 0.0, 2.0]], F)
    mn, mx = so.train(X)
    gpu_or_skip()
    enc = sq8.train(X)
    b = enc.GetBounds()
    assert _same(b[0], mn) and _same(b[1], mx) and np.isnan(b[0][0]) and np.isnan(b[1][0])
    assert np.array_equal(enc.Encode(X), so.encode(X, mn, mx))
    allc = np.arange(256, dtype=np.uint8).repeat(3).reshape(256, 3)
    assert _same(enc.Decode(allc), so.decode(allc, mn, mx))
    enc.Close()
    # a constant column trains at 1.0 and fails at 2.0 with the reference's text; a failed training leaves the handle untrained
    enc = _enc(2)
    with pytest.raises(_lib.LongbowGPUError, match="min must be less than max for all dimensions") as ei:
        enc.train(np.full((3, 2), 2.0, F))
    assert ei.value.code == 1 and not enc.trained
    with pytest.raises(_lib.LongbowGPUError, match="no vectors provided for training") as ei:
        enc.train(np.zeros((0, 2), F))
    assert ei.value.code == 1
    enc.train(np.full((3, 2), 1.0, F))
    b = enc.GetBounds()
    assert (b[0] == F(1.0)).all() and (b[1] == F(1.0) + F(1e-7)).all()
    with pytest.raises(_lib.LongbowGPUError, match="min must be less than max") as ei:
        enc.set_bounds([0.0, 1.0], [1.0, 1.0])
    assert ei.value.code == 1
    b = enc.GetBounds()  # a refused set_bounds changes nothing
    assert (b[0] == F(1.0)).all()
    enc.Close()
    # +0 and -0 in one column: the bound compares equal to the oracle's
    Z = np.array([[-0.0, 0.0, 0.3], [0.0, -0.0, -0.2], [0.7, -0.5, 0.0], [-0.3, 0.2, -0.0]], F)
    for data in (Z, Z[::-1].copy()):
        enc = sq8.train(data)
        mn, mx = so.train(data)
        b = enc.GetBounds()
        assert np.array_equal(b[0], mn) and np.array_equal(b[1], mx)
        assert np.array_equal(enc.Encode(Z), so.encode(Z, mn, mx))
        enc.Close()


@pytest.mark.parametrize("dims", [5, 100])
def test_codec_special_values(dims):
    tiny = F(1e-45)
    vals = np.array([np.nan, -np.nan, np.inf, -np.inf, tiny, -tiny, np.finfo(F).tiny, -np.finfo(F).tiny, 0.0, -0.0, 1.0, -1.0, 0.5,
                     np.finfo(F).max, -np.finfo(F).max], F)
    X = np.stack([np.resize(np.roll(vals, s), dims) for s in range(vals.size)])
    cases = [
        (np.full(dims, -1.0, F), np.full(dims, 1.0, F)),
        (np.zeros(dims, F), np.full(dims, 2.0 ** -119, F)),          # a denormal v - min under a large scale: not flushed
        (np.zeros(dims, F), np.full(dims, 1e-45, F)),                # scale overflows: inf and NaN products give 0
        (np.full(dims, -np.inf, F), np.full(dims, np.inf, F)),       # infinite bounds pass Validate
        (np.full(dims, -np.finfo(F).max, F), np.full(dims, np.finfo(F).max, F)),  # max - min overflows: scale 0
    ]
    den = np.array([0.0, 0.75 * 2.0 ** -126, 2.0 ** -120, 2.0 ** -119, 2.0 ** -121, 1.5 * 2.0 ** -127], F)
    Xd = np.stack([np.resize(np.roll(den, s), dims) for s in range(den.size)])
    assert so.encode(Xd, *cases[1]).max() == 255 and (so.encode(Xd, *cases[1]) == 1).any()
    allc = np.arange(256, dtype=np.uint8).repeat(dims).reshape(256, dims)
    for mn, mx in cases:
        enc = _enc(dims)
        enc.set_bounds(mn, mx)
        for V in (X, Xd):
            assert np.array_equal(enc.Encode(V), so.encode(V, mn, mx))
        assert _same(enc.Decode(allc), so.decode(allc, mn, mx))
        enc.add_vectors(X)
        assert np.array_equal(enc.get_codes(), so.encode(X, mn, mx))
        enc.Close()


@pytest.mark.parametrize("dims", [16, 100])
def test_device_pointer_codec_and_adds_equal_the_host_forms(dims):
    import torch
    n = 777
    enc = _enc(dims)
    rng = np.random.default_rng(3)
    X = (rng.random((n, dims), dtype=F) * F(2) - F(1)).astype(F)
    mn, mx = so.train(X[:500])
    enc.set_bounds(mn, mx)
    want = so.encode(X, mn, mx)
    dX = torch.from_numpy(X).cuda()
    dC = torch.full((n, dims), 0x5A, dtype=torch.uint8, device="cuda")
    enc.encode_device(n, dX.data_ptr(), dC.data_ptr())
    assert np.array_equal(dC.cpu().numpy(), want)
    enc.add_vectors_device(n, dX.data_ptr())
    enc.add_codes_device(n, dC.data_ptr())
    enc.add_vectors(X[:5])
    enc.add_codes(want[:3])
    assert enc.ntotal == 2 * n + 8
    assert np.array_equal(enc.get_codes(), np.concatenate([want, want, want[:5], want[:3]]))
    assert np.array_equal(enc.get_codes(n - 1, 3), np.concatenate([want[-1:], want[:2]]))
    enc.Close()


def test_golden_cases_through_the_library():
    k = so.load_kats()
    e = k["encode"]
    enc = _enc(4)
    enc.set_bounds(e["min"], e["max"])
    for c in e["cases"]:
        assert enc.Encode(F(c["input"])).tolist() == c["expect"], c["name"]
    for c in k["decode_ranges"]["cases"]:
        v = enc.Decode(np.uint8(c["input"]))
        assert ((v >= F(c["lo"])) & (v <= F(c["hi"]))).all(), c["name"]
    t = k["distance"]
    q1, q2, q3 = (enc.Encode(F(t[n])) for n in ("v1", "v2", "v3"))
    assert enc.SQ8EuclideanDistance(q1, q1) <= t["d11_max"]
    assert t["d12"][0] <= enc.SQ8EuclideanDistance(q1, q2) <= t["d12"][1]
    assert t["d13"][0] <= enc.SQ8EuclideanDistance(q1, q3) <= t["d13"][1]
    assert t["d23"][0] <= enc.SQ8EuclideanDistance(q2, q3) <= t["d23"][1]
    for c in k["distance_fast"]["cases"]:
        assert enc.SQ8DistanceFast(np.uint8(c["a"]), np.uint8(c["b"])) == c["expected"]
    enc.Close()
    z = k["quantize"]
    enc = _enc(len(z["src"]))
    enc.set_bounds(np.full(len(z["src"]), z["min"], F), np.full(len(z["src"]), z["max"], F))
    assert enc.Encode(F(z["src"])).tolist() == z["expect"]
    enc.Close()
    for c in k["euclidean_sizes"]["cases"]:
        if c["size"] == 0:
            continue  # (a handle has at least one dimension: the empty case is the oracle's alone)
        enc = _enc(c["size"])
        assert enc.SQ8DistanceFast(c["a"], c["b"]) == c["expected"], c["name"]
        assert enc.EuclideanDistanceSQ8Batch(c["a"], c["b"].reshape(1, -1)).tolist() == [float(F(c["expected"]))], c["name"]
        enc.Close()


def test_untrained_and_retrain_refusals():
    from longbow_amd import _lib
    dims = 20
    enc = _enc(dims)
    rng = np.random.default_rng(4)
    X = rng.random((10, dims), dtype=F)
    codes = rng.integers(0, 256, (10, dims), dtype=np.uint8)
    for call in (lambda: enc.Encode(X), lambda: enc.Decode(codes), lambda: enc.add_vectors(X), lambda: enc.search(X, 3),
                 lambda: enc.GetBounds(), lambda: enc.rerank(codes[0], [0], want_euclid=True)):
        with pytest.raises(_lib.LongbowGPUError, match="config must be trained") as ei:
            call()
        assert ei.value.code == 1
    # INVALID_ARG (untrained) before UNSUPPORTED (k): nothing is written
    d = np.full(10 * 2049, 9.0, F)
    l = np.full(10 * 2049, 77, np.int64)
    assert enc._lib.lb_gpu_sq8_search(enc._h, 10, X.ctypes.data, 2049, d.ctypes.data, l.ctypes.data) == 1
    assert (d == 9.0).all() and (l == 77).all()
    # codes alone need no bounds
    enc.add_codes(codes)
    assert np.array_equal(enc.get_codes(), codes)
    assert np.array_equal(enc.distance_batch(codes[1]), so.dist_s(codes[1], codes))
    assert np.array_equal(enc.rerank(codes[1], [2, 0], want_euclid=False), so.dist_s(codes[1], codes[[2, 0]]))
    _check_search(enc, codes[:2], codes, [3])
    assert enc._lib.lb_gpu_sq8_search_codes(enc._h, 2, codes.ctypes.data, 2049, d.ctypes.data, l.ctypes.data) == 6
    assert b"2049" in enc._lib.lb_gpu_sq8_last_error(enc._h)
    assert enc._lib.lb_gpu_sq8_reserve(enc._h, 1 << 31) == 6
    assert enc._lib.lb_gpu_sq8_get_codes(enc._h, 9, 2, d.ctypes.data) == 1
    assert (d == 9.0).all() and (l == 77).all()
    # the bounds cannot change once rows are stored
    for call in (lambda: enc.train(X), lambda: enc.set_bounds(np.zeros(dims, F), np.ones(dims, F))):
        with pytest.raises(_lib.LongbowGPUError, match="once rows are stored") as ei:
            call()
        assert ei.value.code == 1
    assert not enc.trained
    enc.Close()


# ---- distance_batch and rerank ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [1, 16, 17, 768, 8192])
def test_distance_batch_and_rerank(dims):
    from longbow_amd import _lib
    n = 300
    rng = np.random.default_rng(dims)
    codes = rng.integers(0, 256, (n, dims), dtype=np.uint8)
    codes[7] = 0
    codes[8] = 255
    q = rng.integers(0, 256, dims, dtype=np.uint8)
    mn = (rng.random(dims, dtype=F) - F(0.5)).astype(F)
    mx = (mn + rng.random(dims, dtype=F) + F(0.01)).astype(F)
    enc = _enc(dims)
    enc.add_codes(codes)
    want = so.dist_s(q, codes)
    got = enc.distance_batch(q)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(enc.distance_batch(q, 5, 260), want[5:265])
    assert np.array_equal(enc.distance_batch(q, n - 1, 1), want[n - 1:])
    assert np.array_equal(enc.EuclideanDistanceSQ8Batch(q), want.astype(F))
    # the largest S: all 0 against all 255
    zero = np.zeros(dims, np.uint8)
    assert int(enc.distance_batch(zero, 8, 1)[0]) == 65025 * dims == int(so.dist_s(zero, codes[8:9])[0])
    assert int(enc.distance_batch(np.full(dims, 255, np.uint8), 7, 1)[0]) == 65025 * dims
    with pytest.raises(_lib.LongbowGPUError):
        enc.distance_batch(q, n - 1, 2)
    rows = np.array([0, n - 1, 7, 8, 8, -1, n, 1 << 40, 255, 256], np.int64)
    ok = (rows >= 0) & (rows < n)
    s = enc.rerank(q, rows, want_euclid=False)
    assert s.dtype == np.int32
    assert np.array_equal(s[ok], want[rows[ok]]) and (s[~ok] == INT32_MAX).all()
    enc.Close()
    twin = _enc(dims)
    twin.set_bounds(mn, mx)
    twin.add_codes(codes)
    s, e = twin.rerank(q, rows)
    assert np.array_equal(s[ok], want[rows[ok]]) and (s[~ok] == INT32_MAX).all()
    assert np.array_equal(e[ok], so.euclid(q, codes[rows[ok]], mn, mx)) and (e[~ok] == FLT_MAX).all()
    assert twin.SQ8EuclideanDistance(q, codes[3]) == so.euclid(q, codes[3:4], mn, mx)[0]
    twin.Close()


def test_empty_handle_and_device_rerank():
    import torch
    from longbow_amd import _lib
    dims = 40
    enc = _enc(dims)
    q = np.arange(dims, dtype=np.uint8)
    assert enc.distance_batch(q).size == 0
    with pytest.raises(_lib.LongbowGPUError):
        enc.distance_batch(q, 0, 1)
    assert enc.rerank(q, [0, 5], want_euclid=False).tolist() == [INT32_MAX, INT32_MAX]
    lab, dist = enc.search_codes(q, 5)
    assert (lab == -1).all() and (dist == FLT_MAX).all()
    assert enc.get_codes().shape == (0, dims)
    rng = np.random.default_rng(6)
    codes = rng.integers(0, 256, (50, dims), dtype=np.uint8)
    enc.add_codes(codes)
    rows = np.array([3, 49, 50, 0], np.int64)
    dq, dr = torch.from_numpy(q).cuda(), torch.from_numpy(rows).cuda()
    ds = torch.zeros(4, dtype=torch.int32, device="cuda")
    enc.rerank_device(dq.data_ptr(), dr.data_ptr(), 4, ds.data_ptr())
    w = so.dist_s(q, codes)
    assert ds.cpu().numpy().tolist() == [int(w[3]), int(w[49]), INT32_MAX, int(w[0])]
    enc.Close()


# ---- search against the oracle ----------------------------------------------------------------------------------------------
_corpora = {}


def _corpus(dims):
    """one corpus of about 20k random rows per dims, its handle and 33 queries with the oracle's order of every row"""
    if dims not in _corpora:
        n = 20011
        rng = np.random.default_rng(1000 + dims)
        codes = rng.integers(0, 256, (n, dims), dtype=np.uint8)
        Q = rng.integers(0, 256, (33, dims), dtype=np.uint8)
        Q[1] = codes[n - 1]
        enc = _enc(dims)
        enc.add_codes(codes)
        S = so.dist_matrix(Q, codes)
        assert np.array_equal(S[:, ::997], np.stack([so.dist_s(q, codes[::997]) for q in Q]))
        order = np.stack([np.lexsort((np.arange(n), s)) for s in S])
        for a in (codes, Q, S, order):
            a.setflags(write=False)
        _corpora[dims] = (enc, codes, Q, S, order)
    return _corpora[dims]


@pytest.mark.parametrize("k", [1, 100, 2048])
@pytest.mark.parametrize("nq", [1, 2, 7, 17, 33])
@pytest.mark.parametrize("dims", [1, 2, 17, 768, 1000])
def test_search_matches_the_oracle(dims, nq, k):
    enc, codes, Q, S, order = _corpus(dims)
    lab, dist = enc.search_codes(Q[:nq], k)
    want = order[:nq, :k]
    assert np.array_equal(lab, want)
    assert np.array_equal(dist, np.take_along_axis(S[:nq], want, axis=1).astype(F))
    if dims == 1 and k > 1:
        assert all(np.unique(d).size < k for d in dist)  # 20011 rows on 256 values: ties are the rule here


# ---- tile and workgroup edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_small_n_pads(n):
    dims, k = 16, 300
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 256, (n, dims), dtype=np.uint8)
    Q = rng.integers(0, 256, (3, dims), dtype=np.uint8)
    enc = _enc(dims)
    enc.add_codes(codes)
    _check_search(enc, Q, codes, [k, 1, 255, 256, 257])
    lab, dist = enc.search_codes(Q, k)
    assert (lab[:, n:] == -1).all() and (dist[:, n:] == FLT_MAX).all() and (lab[:, :n] >= 0).all()
    enc.Close()


def test_search_where_a_workgroup_walks_several_tiles():
    # more than 2 * MAX_BLOCKS tiles (the grid cap, SQ8_MAX_BLOCKS = 1024): each workgroup owns a run of 3 tiles
    dims = 16
    n = 2 * MAX_BLOCKS * TILE + 77
    run = 3 * TILE
    rng = np.random.default_rng(8)
    codes = rng.integers(0, 256, (n, dims), dtype=np.uint8)
    Q = rng.integers(0, 256, (2, dims), dtype=np.uint8)
    # the first query's nearest rows: in the first tile, across a tile boundary, across a workgroup boundary, in the last
    # partial tile; exact copies (S = 0) and near copies
    planted = [0, 5, TILE - 1, TILE, run - 1, run, 100 * run + TILE, n - 30, n - 1]
    for j, r in enumerate(planted):
        codes[r] = Q[0]
        if j % 2:
            codes[r, j % dims] ^= 1  # S = 1
    enc = _enc(dims)
    enc.add_codes(codes)
    S = so.dist_matrix(Q, codes)
    order = [np.lexsort((np.arange(n), s)) for s in S]
    assert sorted(order[0][:len(planted)].tolist()) == sorted(planted)
    for k in (1, 9, 100):
        lab, dist = enc.search_codes(Q, k)
        for i in range(2):
            o = order[i][:k]
            assert np.array_equal(lab[i], o) and np.array_equal(dist[i], S[i][o].astype(F))
    assert np.array_equal(enc.distance_batch(Q[1]), S[1])
    assert np.array_equal(enc.distance_batch(Q[1], TILE + 3, n - TILE - 3), S[1][TILE + 3:])
    enc.Close()


# The scan of the per-workgroup counts (countsel_scan_kernel, shared with the BQ index) gives each of its 256 threads
# ceil(nblk / 256) workgroups.  70,145 rows are 275 tiles, one workgroup each: two per thread, and the last occupied thread owns
# the single workgroup 274, whose tile holds one row.
_SCAN_N = 70145
assert -(-_SCAN_N // TILE) == 275 and _SCAN_N % TILE == 1 and 275 <= MAX_BLOCKS


def test_search_scan_gives_a_thread_two_workgroups():
    # Three distinct codes at dims 1 assigned at random, the last row among the first's: with the three as queries the rows at
    # the threshold (S = 0) lie in nearly every workgroup, and the last one is the last row of the corpus.  A fourth code on
    # about one row in 70 and as the fourth query: at k = 2048 its thousand rows are the rows BELOW the threshold, a few in
    # most workgroups, so the scan of both counts is pinned.
    rng = np.random.default_rng(_SCAN_N)
    four = rng.choice(256, 4, replace=False).astype(np.uint8).reshape(4, 1)
    which = rng.integers(0, 3, _SCAN_N)
    which[rng.random(_SCAN_N) < 1 / 70] = 3
    which[-1] = 0
    assert 100 < (which == 3).sum() < 2048 and np.unique(np.flatnonzero(which == 3) // TILE).size > 200
    codes = four[which]
    enc = _enc(1)
    enc.add_codes(codes)
    _check_search(enc, four, codes, [100, 2048], ctx="three values and a sparse fourth")
    enc.Close()


# ---- the three radix digits -------------------------------------------------------------------------------------------------
def _digit_rows(a, b, c):
    """rows at dims 8192 whose S against the zero query is a * 2^21 + b * 2^10 + c: 128 a bytes of 128, b bytes of 32, c of 1"""
    dims = 8192
    rows = np.zeros((len(a), dims), np.uint8)
    for r, (x, y, z) in enumerate(zip(a, b, c)):
        assert 128 * x + y + z <= dims
        rows[r, :128 * x] = 128
        rows[r, 128 * x:128 * x + y] = 32
        rows[r, 128 * x + y:128 * x + y + z] = 1
    return rows


@pytest.mark.parametrize("digit", ["top", "middle", "low"])
def test_each_radix_digit_decides(digit):
    n = 600
    rng = np.random.default_rng(len(digit))
    a, b, c = np.full(n, 3), np.full(n, 9), np.full(n, 7)
    if digit == "top":
        a = rng.integers(0, 41, n)       # S differs in bits 21 and up only
    elif digit == "middle":
        b = rng.integers(0, 501, n)      # bits 10..20 only
    else:
        c = rng.integers(0, 1001, n)     # bits 0..9 only
    codes = _digit_rows(a, b, c)
    zero = np.zeros(8192, np.uint8)
    S = so.dist_s(zero, codes)
    assert np.array_equal(S, a * (1 << 21) + b * (1 << 10) + c)
    diff = np.bitwise_or.reduce(S ^ S[0])
    assert {"top": diff >> 21 != 0 and diff & ((1 << 21) - 1) == 0,
            "middle": diff >> 21 == 0 and diff & 1023 == 0 and diff != 0,
            "low": diff >> 10 == 0 and diff != 0}[digit]
    Q = np.stack([zero, rng.integers(0, 256, 8192, dtype=np.uint8)])
    enc = _enc(8192)
    enc.add_codes(codes)
    srt = np.sort(S)
    ks = set()
    for t in (srt[0], srt[n // 3], srt[n - 1]):  # k around count(< t) and count(<= t)
        lt, le = int((S < t).sum()), int((S <= t).sum())
        ks |= {lt - 1, lt, lt + 1, le - 1, le, le + 1}
    _check_search(enc, Q, codes, sorted(k for k in ks if 1 <= k <= 2048), ctx=digit)
    enc.Close()


# ---- ties -------------------------------------------------------------------------------------------------------------------
def test_identical_rows():
    dims, n = 33, 700
    row = np.arange(dims, dtype=np.uint8) * 7
    codes = np.tile(row, (n, 1))
    enc = _enc(dims)
    enc.add_codes(codes)
    Q = np.stack([row, np.zeros(dims, np.uint8)])
    for k in (1, n - 1, n, n + 1, 2048):
        lab, dist = enc.search_codes(Q, k)
        m = min(k, n)
        assert np.array_equal(lab[:, :m], np.tile(np.arange(m), (2, 1))) and (lab[:, m:] == -1).all()
        assert (dist[0, :m] == 0).all() and (dist[1, :m] == F(int(so.dist_s(Q[1], codes[:1])[0]))).all() and (dist[:, m:] == FLT_MAX).all()
    enc.Close()


def test_interleaved_ties_go_to_the_lowest_positions():
    # dims 2, query (0, 0): (3, 4) and (5, 0) are both at S = 25, (6, 0) at 36, (1, 1) at 2
    n = 1000
    codes = np.zeros((n, 2), np.uint8)
    codes[0::4] = (3, 4)
    codes[1::4] = (6, 0)
    codes[2::4] = (5, 0)
    codes[3::4] = (0, 6)
    codes[[10, 500, 999]] = (1, 1)
    Q = np.array([[0, 0], [6, 0]], np.uint8)
    enc = _enc(2)
    enc.add_codes(codes)
    _check_search(enc, Q, codes, [1, 2, 3, 4, 10, 333, 499, 500, 501, 502, 999, 1000, 1001])
    enc.Close()


def test_float32_of_s_merges_two_distances_but_the_order_is_the_integers():
    dims = 300
    base = 258 * 65025

    def row(extra):
        r = np.zeros(dims, np.uint8)
        r[:258] = 255
        i = 258
        while extra > 0:
            d = min(255, int(np.sqrt(extra)))
            r[i] = d
            extra -= d * d
            i += 1
        return r
    codes = np.stack([row(s - base) for s in ((1 << 24) + 1, 1 << 24, (1 << 24) + 2, (1 << 24) + 1)])
    q = np.zeros(dims, np.uint8)
    enc = _enc(dims)
    enc.add_codes(codes)
    assert enc.distance_batch(q).tolist() == [(1 << 24) + 1, 1 << 24, (1 << 24) + 2, (1 << 24) + 1]
    lab, dist = enc.search_codes(q, 4)
    assert lab[0].tolist() == [1, 0, 3, 2]
    assert dist[0].tolist() == [float(1 << 24)] * 3 + [float((1 << 24) + 2)]
    enc.Close()


# ---- other ------------------------------------------------------------------------------------------------------------------
def test_more_queries_than_one_scratch_batch():
    # A batch holds at most 1024 queries, and no more than fit 1 GiB of int32 distances (n above 2^18 rows lowers it; a
    # corpus of that size does not belong here): 1025 queries are two batches over the same scratch at any n.
    dims, n, nq = 4, 300, 1025
    rng = np.random.default_rng(12)
    codes = rng.integers(0, 256, (n, dims), dtype=np.uint8)
    Q = rng.integers(0, 256, (nq, dims), dtype=np.uint8)
    enc = _enc(dims)
    enc.add_codes(codes)
    lab, dist = enc.search_codes(Q, 5)
    olab, odist = so.search(Q, codes, 5)
    assert np.array_equal(lab, olab) and np.array_equal(dist, odist)
    enc.Close()


def test_growth_keeps_positions():
    dims = 17
    rng = np.random.default_rng(13)
    codes = rng.integers(0, 256, (11000, dims), dtype=np.uint8)
    enc = _enc(dims)
    enc.add_codes(codes[:3000])            # the first allocation: 4096 rows
    enc.add_codes(codes[3000:6000])        # grows to 8192: the rows move
    enc.reserve(9000)                      # and again
    enc.add_codes(codes[6000:])
    assert enc.ntotal == 11000 and np.array_equal(enc.get_codes(), codes)
    Q = codes[[0, 2999, 3000, 10999]].copy()
    Q[:, 0] ^= 3
    _check_search(enc, Q, codes, [1, 50])
    enc.Close()


def test_f32_search_entry_points_and_cancellation():
    import torch
    from longbow_amd import _lib, gpu
    dims, n, nq, k = 100, 4000, 5, 20
    rng = np.random.default_rng(21)
    X = (rng.random((n, dims), dtype=F) - F(0.5)).astype(F)
    Q = (rng.random((nq, dims), dtype=F) - F(0.5)).astype(F)
    enc = _enc(dims)
    enc.train(X)
    mn, mx = so.train(X)
    enc.add_vectors(X)
    lab, dist = enc.search(Q, k)
    clab, cdist = enc.search_codes(enc.Encode(Q), k)
    olab, odist = so.search(so.encode(Q, mn, mx), so.encode(X, mn, mx), k)
    assert np.array_equal(lab, clab) and np.array_equal(dist, cdist)
    assert np.array_equal(lab, olab) and np.array_equal(dist, odist)
    dQ = torch.from_numpy(Q).cuda()
    dD = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    dL = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    enc.search_device(nq, dQ.data_ptr(), k, dD.data_ptr(), dL.data_ptr())
    assert np.array_equal(dL.cpu().numpy(), lab) and np.array_equal(dD.cpu().numpy(), dist)
    # a fired context: LB_ERR_CANCELLED, nothing is launched, nothing is written
    ctx = gpu.Cancel()
    ctx.fire()
    with pytest.raises(_lib.Canceled) as ei:
        enc.search(Q, k, ctx=ctx)
    assert ei.value.code == 8
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
    enc.Close()


def test_search_rerank_composition(oracle):
    from longbow_amd import sq8
    n, dims, nq, k, over = 5000, 64, 4, 10, 10
    rng = np.random.default_rng(77)
    X = (rng.random((n, dims), dtype=F) - F(0.5)).astype(F)
    Q = (X[rng.integers(0, n, nq)] + F(0.05) * (rng.random((nq, dims), dtype=F) - F(0.5))).astype(F)
    gpu_or_skip()
    enc = sq8.train(X)
    mn, mx = so.train(X)
    enc.add_vectors(X)
    idx = new_index(dims, 0)
    idx.Add(None, X)
    lab, dist = sq8.search_rerank(enc, idx, Q, k, over)
    short, _ = so.search(so.encode(Q, mn, mx), so.encode(X, mn, mx), k * over)
    for i in range(nq):
        d = oracle.batch_flat(0, Q[i], X[short[i]], 1)
        keep = np.lexsort((short[i], d))[:k]
        assert np.array_equal(lab[i], short[i][keep]) and np.array_equal(dist[i], d[keep])
    assert np.array_equal(enc.search_rerank(idx, Q, k, over)[0], lab)
    idx.Close()
    enc.Close()
