"""lb_gpu_pq4_* on the GPU against the oracle, bit for bit: the reference's K <= 16 arithmetic (oracle.pq_encode's
encodeSequential branch, build_adc_table and adc_single at stride 16) under the batch form's float32(sqrt(float64(s)))."""
import numpy as np
import pytest

from tests.gpu_util import diag_lib, gpu_or_skip

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(F).max
WG_ROWS = 4 * 64          # PQ4_WAVES * 64 (lb_pq4.h): the rows of one workgroup of the scan
SAMPLE_MIN_ROWS = 65536   # kAdcSampleMinRows (lb_handle.h): from here on a search leaves boot mode for the sampled threshold


def _enc(cb, lib=None):
    from longbow_amd import pq, pq4
    return pq4.PQ4Encoder(pq.serialize_codebooks(cb), lib=lib)


def _ref_dist(oracle, cb, q, pool, idx):
    """distances of the rows pool[idx] to q: adc_single once per distinct row of the pool"""
    table = oracle.build_adc_table(cb, q)
    s = np.array([oracle.adc_single(table, c, 16) for c in pool], F)
    with np.errstate(invalid="ignore"):
        return np.sqrt(s.astype(np.float64)).astype(F)[idx]


def _ref_topk(d, k):
    order = np.argsort(d, kind="stable")[:k]  # ascending (distance, row), NaN last
    lab, dist = np.full(k, -1, np.int64), np.full(k, FLT_MAX, F)
    lab[:order.size], dist[:order.size] = order, d[order]
    return lab, dist


@pytest.mark.parametrize("kind", ["dup", "inf", "nan"])
@pytest.mark.parametrize("M,sub", [(1, 1), (3, 5), (32, 4), (96, 8)])
def test_encode_and_add_vectors(oracle, M, sub, kind):
    gpu_or_skip()
    rng = np.random.default_rng(M * 100 + sub)
    cb = rng.random((M, 16, sub), dtype=F)
    if kind == "dup":
        cb[:, 5] = cb[:, 2]            # duplicate centroids: the first wins
        cb[:, 0] = cb[:, 2]
    else:
        cb[M - 1] = np.inf if kind == "inf" else np.nan  # no distance below FLT_MAX: code 0
    V = rng.random((300, M * sub), dtype=F)
    V[:16, :sub] = cb[0, :, :sub] if kind == "dup" else V[:16, :sub]  # exact hits on (duplicated) centroids
    enc = _enc(cb)
    want = np.stack([oracle.pq_encode(cb, v) for v in V])
    if kind != "dup":
        assert (want[:, M - 1] == 0).all()
    assert np.array_equal(enc.Encode(V), want)
    assert np.array_equal(enc.Encode(V[7]), want[7])
    enc.add_vectors(V)
    assert enc.ntotal == 300 and np.array_equal(enc.get_codes(), want)
    enc.Close()


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("M", [1, 3, 32, 34])
def test_pack_round_trip(M, n):
    gpu_or_skip()
    rng = np.random.default_rng(M * 1000 + n)
    enc = _enc(rng.random((M, 16, 2), dtype=F))
    codes = rng.integers(0, 16, (n, M), dtype=np.uint8)
    enc.add_codes(codes)
    assert enc.ntotal == n and np.array_equal(enc.get_codes(), codes)
    assert np.array_equal(enc.get_codes(n - 1, 1), codes[n - 1:])
    assert enc.hbm_bytes == 4096 * ((M + 1) // 2) + M * 16 * 2 * 4  # the first allocation holds 4096 packed rows
    enc.Close()


def test_adds_across_a_growth_and_a_refused_batch():
    import torch
    from longbow_amd import _lib
    gpu_or_skip()
    rng = np.random.default_rng(5)
    M = 3
    enc = _enc(rng.random((M, 16, 2), dtype=F))
    codes = rng.integers(0, 16, (4300, M), dtype=np.uint8)
    enc.add_codes(codes[:4000])
    enc.add_codes(codes[4000:])  # 4096 rows were allocated: this add grows the buffer
    assert np.array_equal(enc.get_codes(), codes)
    bad = rng.integers(0, 16, (70, M), dtype=np.uint8)
    bad[69, 2] = 16
    for add in (lambda: enc.add_codes(bad), lambda: enc.add_codes_device(70, torch.from_numpy(bad).cuda().data_ptr())):
        with pytest.raises(_lib.LongbowGPUError, match="16 or more") as e:
            add()
        assert e.value.code == 1 and enc.ntotal == 4300 and np.array_equal(enc.get_codes(), codes)
    enc.add_codes_device(69, torch.from_numpy(bad[:69].copy()).cuda().data_ptr())
    assert np.array_equal(enc.get_codes(4300), bad[:69])
    enc.Close()


@pytest.mark.parametrize("M", [3, 32, 96, 160])  # the generic form (registers), the fast form at one and three KiB a run, the chunked LDS form
def test_adc_distance_batch(oracle, M):
    gpu_or_skip()
    rng = np.random.default_rng(M)
    cb = rng.random((M, 16, 2), dtype=F)
    codes = rng.integers(0, 16, (300, M), dtype=np.uint8)
    enc = _enc(cb)
    enc.add_codes(codes)
    q = rng.random(M * 2, dtype=F)
    table = enc.BuildADCTable(q)
    assert np.array_equal(table, oracle.build_adc_table(cb, q))
    want = _ref_dist(oracle, cb, q, codes, np.arange(300))
    for row0 in (0, 1, 65):
        for n in (1, 64, 200):
            got = np.full(n + 1, -1, F)
            enc.ADCDistanceBatch(table, got[:n], row0=row0)
            assert np.array_equal(got[:n], want[row0:row0 + n]) and got[n] == -1, (row0, n)
    enc.Close()


@pytest.mark.parametrize("M,sub,n,nq,k", [
    (3, 5, 1, 1, 1),
    (3, 5, 64, 2, 10),
    (32, 4, 65, 5, 70),                     # k = n + 5; four queries in a pass and a remainder
    (32, 4, WG_ROWS + 1, 1, 10),
    (96, 8, WG_ROWS + 1, 5, 10),
    (160, 2, 65, 2, 10),
    (160, 2, WG_ROWS + 1, 5, WG_ROWS + 6),  # the LDS form: two pairs and a single
    (96, 8, SAMPLE_MIN_ROWS - 1, 2, 4096),  # boot mode, several chunks
    (96, 8, SAMPLE_MIN_ROWS + 500, 5, 50),  # the sampled threshold (a plan exists for k up to about 90 at this size)
    (3, 5, 70000, 1, 10),
    (160, 2, SAMPLE_MIN_ROWS + 500, 2, 10),
    (32, 4, SAMPLE_MIN_ROWS + 500, 1, 4096),
])
def test_search(oracle, M, sub, n, nq, k):
    gpu_or_skip()
    rng = np.random.default_rng(M + n + k)
    cb = rng.random((M, 16, sub), dtype=F)
    pool = rng.integers(0, 16, (min(n, 3000), M), dtype=np.uint8)  # large corpora repeat 3000 distinct rows
    idx = np.arange(n) if n <= 3000 else rng.integers(0, 3000, n)
    enc = _enc(cb)
    enc.add_codes(pool[idx])
    Q = rng.random((nq, M * sub), dtype=F)
    lab, dist = enc.Search(Q, k)
    for b in range(nq):
        wl, wd = _ref_topk(_ref_dist(oracle, cb, Q[b], pool, idx), k)
        assert np.array_equal(lab[b], wl) and np.array_equal(dist[b], wd), b
    enc.Close()


@pytest.mark.parametrize("M,nq", [(32, 5), (96, 5), (128, 2), (128, 1)])
def test_register_lookup_in_the_fast_form(oracle, monkeypatch, M, nq):
    """Rows that take the fast form are looked up in LDS by default (the faster of the two); the diagnostic build's
    LB_PQ4_LOOKUP=0 serves them from registers, four queries a pass up to M = 96 and two beyond."""
    monkeypatch.setenv("LB_PQ4_LOOKUP", "0")
    rng = np.random.default_rng(M + nq)
    cb = rng.random((M, 16, 2), dtype=F)
    codes = rng.integers(0, 16, (WG_ROWS + 1, M), dtype=np.uint8)
    enc = _enc(cb, lib=diag_lib())
    enc.add_codes(codes)
    Q = rng.random((nq, M * 2), dtype=F)
    lab, dist = enc.Search(Q, 10)
    for b in range(nq):
        d = _ref_dist(oracle, cb, Q[b], codes, np.arange(WG_ROWS + 1))
        wl, wd = _ref_topk(d, 10)
        assert np.array_equal(lab[b], wl) and np.array_equal(dist[b], wd), b
    got = np.empty(200, F)
    enc.ADCDistanceBatch(enc.BuildADCTable(Q[0]), got, row0=1)
    assert np.array_equal(got, _ref_dist(oracle, cb, Q[0], codes, np.arange(1, 201)))
    enc.Close()


def test_ties_keep_the_lowest_rows(oracle):
    gpu_or_skip()
    rng = np.random.default_rng(11)
    cb = rng.random((32, 16, 2), dtype=F)
    pool = rng.integers(0, 16, (3, 32), dtype=np.uint8)
    idx = np.arange(5000) % 3
    enc = _enc(cb)
    enc.add_codes(pool[idx])
    q = rng.random(64, dtype=F)
    lab, dist = enc.Search(q, 100)
    d = _ref_dist(oracle, cb, q, pool, idx)
    wl, wd = _ref_topk(d, 100)
    assert np.array_equal(wl, np.arange(5000)[idx == np.argmin(d[:3])][:100])  # the lowest rows of the nearest code row
    assert np.array_equal(lab[0], wl) and np.array_equal(dist[0], wd)
    enc.Close()


def test_non_finite_distances_come_last(oracle):
    gpu_or_skip()
    rng = np.random.default_rng(12)
    cb = rng.random((3, 16, 5), dtype=F)
    cb[0, 3, 1], cb[2, 9, 4] = np.inf, np.nan
    codes = rng.integers(0, 16, (300, 3), dtype=np.uint8)
    enc = _enc(cb)
    enc.add_codes(codes)
    q = rng.random(15, dtype=F)
    lab, dist = enc.Search(q, 300)
    wl, wd = _ref_topk(_ref_dist(oracle, cb, q, codes, np.arange(300)), 300)
    n_nan, n_inf = int((codes[:, 2] == 9).sum()), int(((codes[:, 0] == 3) & (codes[:, 2] != 9)).sum())
    assert n_nan > 0 and n_inf > 0
    assert np.isnan(wd[300 - n_nan:]).all() and np.isposinf(wd[300 - n_nan - n_inf:300 - n_nan]).all() and np.isfinite(wd[:300 - n_nan - n_inf]).all()
    assert np.array_equal(lab[0], wl) and np.array_equal(dist[0], wd, equal_nan=True)
    enc.Close()


def test_refused_k_and_cancellation():
    from longbow_amd import _lib, gpu
    lib = gpu_or_skip()
    rng = np.random.default_rng(13)
    enc = _enc(rng.random((3, 16, 2), dtype=F))
    enc.add_codes(rng.integers(0, 16, (100, 3), dtype=np.uint8))
    q = rng.random((1, 6), dtype=F)
    dist, lab = np.full(4097, 9.0, F), np.full(4097, 77, np.int64)
    assert lib.lb_gpu_pq4_search(enc._h, 1, q.ctypes.data, 4097, dist.ctypes.data, lab.ctypes.data) == 6  # LB_ERR_UNSUPPORTED
    assert (dist == 9.0).all() and (lab == 77).all()
    ctx = gpu.Cancel()
    ctx.fire()
    with pytest.raises(_lib.Canceled):
        enc.Search(q, 5, ctx=ctx)
    assert enc.Search(q, 5)[0].shape == (1, 5)
    enc.Close()
