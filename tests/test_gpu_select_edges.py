"""The data-dependent branches of the radix k-th selection and of the result emit (csrc/lb_select.h: radix_kth, compact_le,
emit_sorted) on their consumers -- the flat f32 index on its batched route (the finish kernels' register form), the flat index
on the exact scan and the PQ handle (select_kernel) -- and of the same walk in ivf_select_kernel's own text (kernels_ivf.hip):
IVF-Flat and IVF-PQ with every list probed.
Labels and distance bits must equal the oracle's: these paths are exact, there is no tolerance.

What decides the routes (read from the code, asserted below through last_route where the handle reports one):
  flat index, fewer than 5 queries (LB_NARROW_MINQ): the exact scan.  Its selects keep kc = k candidates; the first one reads a
      bootstrap chunk of up to 8192 rows, so an index of n <= 8192 rows is selected in one go: bitonic for next_pow2(n) <=
      2 next_pow2(k), radix beyond.  Up to 8 queries a launch: the 1024-thread form.
  flat index, 5 queries or more at a dimension that is a multiple of 32: a candidate route.  Its selects keep kc =
      next_pow2(max(2k, k + 32, 64)) candidates (cand_geometry: 64 at k = 1 and 10, 256 at k = 100) unsorted; below 16,384 rows
      there is no sampled threshold, the bootstrap chunk is max(4 kc, 2048) rows, and the finish kernel ends the search.  One
      workgroup per query of the batch: 1024 threads up to 512 queries (LB_SELECT_BIG_MAXQ), 256 threads beyond.
  PQ handle: select_kernel with kc = k, one query a launch.
  IVF handles: ivf_select_kernel, Pk = next_pow2(k); bitonic for next_pow2(n) <= 2 Pk, radix beyond."""
import numpy as np
import pytest

from tests import ivfpq_oracle as pqo
from tests.gpu_util import assert_same, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = np.finfo(F).max
DIM = 32              # flat and IVF-Flat rows
PQ_DIM, PQ_M = 8, 4   # PQ and IVF-PQ rows
N = 3000
NQ_SCAN, NQ_BATCHED = 2, 6
KS = (1, 10, 100)


def _centroids(dim):
    return np.stack([np.zeros(dim, F), np.ones(dim, F), -np.ones(dim, F)])


def _ids(n):
    return np.random.default_rng(n).permutation(1 << 22)[:n].astype(np.int64) + (1 << 41)


# ---- the consumers: each asserts equality with the oracle and returns what it got ----------------------------------------------
def check_flat(oracle, X, Q, k, metric=0, ids=None, routes=("scan", "batched"), ctx=""):
    """-> {route: (labels, dist, candidate route reported)}; Q has at least NQ_BATCHED rows"""
    gpu_or_skip()
    idx = new_index(X.shape[1], metric)
    idx.Add(ids, X)
    out = {}
    for route in routes:
        q = Q[:NQ_SCAN] if route == "scan" else Q
        ol, od = oracle.search_batch(metric, q, X, k, ids=ids, nthreads=4)
        lab, dist = idx.SearchBatch(q, k)
        assert_same(lab, dist, ol, od, f"flat {route} {ctx}")
        out[route] = (lab, dist, idx.last_route[0])
    idx.Close()
    return out


def check_ivf(oracle, X, Q, k, metric=0, ids=None, ctx=""):
    from longbow_amd import ivf
    gpu_or_skip()
    C_ = _centroids(X.shape[1])
    h = ivf.IVFFlat(C_, metric, 0)
    h.add(X, ids)
    ol, od = oracle.search_batch(metric, Q, X, k, ids=ids, nthreads=4)
    lab, dist = h.search(Q, k, C_.shape[0])
    assert_same(lab, dist, ol, od, f"ivf-flat {ctx}")
    assert h.last_search_stats()[1] == Q.shape[0] * X.shape[0]  # every row of every list was scanned
    h.Close()
    return lab, dist


def check_pq(oracle, cb, X, Q, k, ctx=""):
    from longbow_amd import pq
    gpu_or_skip()
    codes = pqo.encode(oracle, cb, X)
    enc = pq.PQEncoder(pqo.blob(cb))
    enc.add_codes(codes)
    ol, od = pqo.brute(oracle, cb, Q, codes, k)
    lab, dist = enc.Search(Q, k)
    assert_same(lab, dist, ol, od, f"pq {ctx}")
    enc.Close()
    return lab, dist


def check_ivfpq(oracle, cb, X, Q, k, ids=None, ctx=""):
    from longbow_amd import ivfpq
    gpu_or_skip()
    C_ = _centroids(X.shape[1])
    codes = pqo.encode(oracle, cb, X)
    h = ivfpq.IVFPQ(pqo.blob(cb), C_, 0)
    h.add(X, ids)
    assert np.array_equal(h.codes(), codes)
    ol, od = pqo.brute(oracle, cb, Q, codes, k)
    if ids is not None:
        ol = np.where(ol >= 0, ids[np.clip(ol, 0, None)], -1)
    lab, dist = h.search(Q, k, C_.shape[0])
    assert_same(lab, dist, ol, od, f"ivf-pq {ctx}")
    assert h.last_search_stats()[1] == Q.shape[0] * X.shape[0]
    h.Close()
    return lab, dist


def check_all(oracle, X, Xpq, cb, Q, Qpq, k, ctx=""):
    """the five consumers on an L2 case -> their (labels, dist), for what the case asserts beyond the oracle"""
    flat = check_flat(oracle, X, Q, k, ctx=ctx)
    assert flat["scan"][2] == 0, f"the {NQ_SCAN}-query search did not take the exact scan {ctx}"
    assert flat["batched"][2] != 0, f"the {NQ_BATCHED}-query batch did not take a candidate route {ctx}"
    return [flat["scan"][:2], flat["batched"][:2], check_ivf(oracle, X, Q, k, ctx=ctx), check_pq(oracle, cb, Xpq, Qpq, k, ctx=ctx),
            check_ivfpq(oracle, cb, Xpq, Qpq, k, ctx=ctx)]


def _random_case(n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, DIM)).astype(F), rng.standard_normal((n, PQ_DIM)).astype(F), pqo.codebooks(PQ_DIM, PQ_M, seed + 1),
            rng.standard_normal((NQ_BATCHED, DIM)).astype(F), rng.standard_normal((NQ_BATCHED, PQ_DIM)).astype(F))


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_all_keys_equal(oracle, k):
    """every row is the same vector: the 32 key bits of all entries agree, the pivot is decided in the row bytes"""
    X, Xpq, cb, Q, Qpq = _random_case(1, seed=11)
    for lab, dist in check_all(oracle, np.tile(X, (N, 1)), np.tile(Xpq, (N, 1)), cb, Q, Qpq, k, ctx=f"k {k}"):
        assert (lab == np.arange(k)).all() and (dist == dist[:, :1]).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------
def _two_shells(k, close, seed):
    """`close` rows at 2.1 .. 2.8 from the origin, the other N - close at 9 .. 30, scattered over the row positions; the queries
    lie within 0.03 of the origin.  A distance of the close group (or its square) lies in [2, 8) whatever the query, a far one
    in [32, 1024) or [8, 32): the sortable keys of the groups differ in their top byte, the first byte counted, and every close
    row falls into one bin of it.  The PQ rows are codebook entries: entries 0 .. 127 of a subspace have squared norms of
    0.55 .. 0.68 (four of them: 2.2 .. 2.72), entries 128 .. 255 of 20 .. 30 (80 .. 120)."""
    rng = np.random.default_rng(seed)
    is_close = np.zeros(N, bool)
    is_close[rng.permutation(N)[:close]] = True

    def shells(dim, lo_c, hi_c, lo_f, hi_f, count, far):
        u = rng.standard_normal((count, dim))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        r = np.where(far, rng.uniform(lo_f, hi_f, count), rng.uniform(lo_c, hi_c, count))
        return (u * r[:, None]).astype(F)

    X = shells(DIM, 2.1, 2.8, 9.0, 30.0, N, ~is_close)
    sub = PQ_DIM // PQ_M
    far_entry = np.tile(np.arange(256) >= 128, PQ_M)
    cb = shells(sub, np.sqrt(0.55), np.sqrt(0.68), np.sqrt(20.0), np.sqrt(30.0), PQ_M * 256, far_entry).reshape(PQ_M, 256, sub)
    codes = rng.integers(0, 128, (N, PQ_M)) + 128 * (~is_close)[:, None]
    Xpq = np.concatenate([cb[m, codes[:, m]] for m in range(PQ_M)], axis=1)
    Q = (rng.standard_normal((NQ_BATCHED, DIM)) * 0.005).astype(F)
    Qpq = (rng.standard_normal((NQ_BATCHED, PQ_DIM)) * 0.005).astype(F)
    return X, Xpq, cb, Q, Qpq, is_close


@pytest.mark.parametrize("extra", [0, 1, -1])
@pytest.mark.parametrize("k", KS)
def test_whole_bucket(oracle, k, extra):
    """exactly k close rows: the first counted byte has need == incl (the whole-bucket shortcut); k + 1: need < incl, the walk
    must descend; k - 1: the k-th result comes from the far group"""
    X, Xpq, cb, Q, Qpq, is_close = _two_shells(k, k + extra, seed=100 * k + extra + 1)
    for lab, dist in check_all(oracle, X, Xpq, cb, Q, Qpq, k, ctx=f"k {k} close rows {k + extra}"):
        got_close = is_close[lab].sum(axis=1)
        assert (got_close == min(k, k + extra)).all(), got_close


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("positive", [5, N // 2])
def test_no_common_leading_byte(oracle, positive):
    """dot metric, distances (-q.x) of both signs: the sortable keys differ in their top bit.  5 rows with a positive score: the
    k-th distance is negative at k = 1 and positive at k = 10 and 100; half of the rows: negative at every k"""
    rng = np.random.default_rng(positive)
    u = rng.standard_normal(DIM)
    u /= np.linalg.norm(u)
    sign = -np.ones(N)
    sign[rng.permutation(N)[:positive]] = 1.0
    X = (np.outer(sign * rng.uniform(0.5, 4.0, N), u) + rng.standard_normal((N, DIM)) * 0.05).astype(F)
    Q = (u + rng.standard_normal((NQ_BATCHED, DIM)) * 0.01).astype(F)
    for k in KS:
        flat = check_flat(oracle, X, Q, k, metric=2, ctx=f"dot k {k}")
        assert flat["scan"][2] == 0 and flat["batched"][2] != 0, "routes"
        res = [flat["scan"][:2], flat["batched"][:2], check_ivf(oracle, X, Q, k, metric=2, ctx=f"dot k {k}")]
        for lab, dist in res:
            assert (dist[:, 0] < 0).all() and ((dist[:, -1] > 0) == (k > positive)).all()


# 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 33])
def test_sort_select_boundary_at_kc_equal_k(oracle, n):
    """k = 10 (next_pow2: 16) where the selection keeps kc = k: 32 entries are sorted whole, 33 take the radix walk -- the IVF
    handles, the flat index's exact scan and the PQ handle"""
    X, Xpq, cb, Q, Qpq = _random_case(n, seed=n)
    flat = check_flat(oracle, X, Q, 10, routes=("scan",), ctx=f"n {n}")
    assert flat["scan"][2] == 0
    check_ivf(oracle, X, Q, 10, ctx=f"n {n}")
    check_pq(oracle, cb, Xpq, Qpq, 10, ctx=f"n {n}")
    check_ivfpq(oracle, cb, Xpq, Qpq, 10, ctx=f"n {n}")


@pytest.mark.parametrize("n", [128, 129])
def test_sort_select_boundary_at_the_candidate_routes_kc(oracle, n):
    """k = 10 on a candidate route: kc = 64 (cand_geometry), and the whole index is the bootstrap chunk -- 128 entries are
    sorted whole, 129 take the radix walk (next_pow2(129) = 256 > 2 * 64)"""
    X, _, _, Q, _ = _random_case(n, seed=n)
    flat = check_flat(oracle, X, Q, 10, routes=("batched",), ctx=f"n {n}")
    assert flat["batched"][2] != 0, "the batch did not take a candidate route"


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9, 10, 11])
def test_few_entries(oracle, n):
    """k = 10 over 1, k - 1, k and k + 1 rows; what is missing is padded with -1 / FLT_MAX"""
    k = 10
    X, Xpq, cb, Q, Qpq = _random_case(n, seed=50 + n)
    flat = check_flat(oracle, X, Q, k, ctx=f"n {n}")
    assert flat["scan"][2] == 0 and flat["batched"][2] != 0, "routes"  # (the finish kernels run at every one of these sizes)
    res = [flat["scan"][:2], flat["batched"][:2], check_ivf(oracle, X, Q, k, ctx=f"n {n}"), check_pq(oracle, cb, Xpq, Qpq, k, ctx=f"n {n}"),
           check_ivfpq(oracle, cb, Xpq, Qpq, k, ctx=f"n {n}")]
    have = min(n, k)
    for lab, dist in res:
        assert (lab[:, :have] >= 0).all() and (dist[:, :have] < FLT_MAX).all()
        assert (lab[:, have:] == -1).all() and (dist[:, have:] == FLT_MAX).all()


# 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [NQ_BATCHED, 520])
def test_both_widths_of_select_kernel(oracle, nq):
    """a candidate route over 3000 rows runs a select behind each of its two chunks (2048 rows, then the rest), one workgroup
    per query of the batch: 1024 threads at 6 queries, 256 threads at 520 (beyond LB_SELECT_BIG_MAXQ = 512); both walk the radix
    path (2048 > 2 * 64)"""
    gpu_or_skip()
    rng = np.random.default_rng(nq)
    X = rng.standard_normal((N, DIM)).astype(F)
    Q = rng.standard_normal((nq, DIM)).astype(F)
    idx = new_index(DIM, 0)
    idx.Add(None, X)
    ol, od = oracle.search_batch(0, Q, X, 10, nthreads=4)
    lab, dist = idx.SearchBatch(Q, 10)
    assert_same(lab, dist, ol, od, f"nq {nq}")
    assert idx.last_route[0] != 0, "the batch did not take a candidate route"
    idx.Close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_ids_present_and_absent(oracle):
    """the emit's two label sources, on every handle that takes ids (the PQ handle has none: its labels are rows)"""
    X, Xpq, cb, Q, Qpq = _random_case(N, seed=7)
    ids, k = _ids(N), 10
    for use in (None, ids):
        flat = check_flat(oracle, X, Q, k, ids=use, ctx=f"ids {use is not None}")
        assert flat["scan"][2] == 0 and flat["batched"][2] != 0, "routes"
        check_ivf(oracle, X, Q, k, ids=use, ctx=f"ids {use is not None}")
        check_ivfpq(oracle, cb, Xpq, Qpq, k, ids=use, ctx=f"ids {use is not None}")
    check_pq(oracle, cb, Xpq, Qpq, k)
