"""uint8 index on the device: labels and distance bits equal to a numpy-float32 restatement of the reference's
euclideanUint8Unrolled4x (four f32 chains, ((s0 + s1) + s2) + s3, sqrt in float64 rounded to float32)."""
import numpy as np
import pytest

from tests.gpu_util import assert_same, gpu_or_skip

pytestmark = pytest.mark.gpu

F, U8 = np.float32, np.uint8
ROUTE_U8_SCAN = 82


def ref_dist(Q, X):
    """[nq, n] float32: the reference's value of every (query, row) pair"""
    QT, XT = np.ascontiguousarray(Q.astype(F).T), np.ascontiguousarray(X.astype(F).T)
    s = [np.zeros((Q.shape[0], X.shape[0]), F) for _ in range(4)]
    dim = Q.shape[1]
    for i in range(dim):
        d = XT[i][None, :] - QT[i][:, None]
        s[i % 4 if i < dim - dim % 4 else 0] += d * d  # (the tail elements go into chain 0)
    return np.sqrt((((s[0] + s[1]) + s[2]) + s[3]).astype(np.float64)).astype(F)


def topk(d, k, rows=None):
    """ascending (value, row); -1 / FLT_MAX padding beyond the rows there are"""
    rows = np.arange(d.size) if rows is None else np.asarray(rows)
    o = np.lexsort((rows, d))[:k]
    lab = np.full(k, -1, np.int64)
    dist = np.full(k, np.finfo(F).max, F)
    lab[:o.size], dist[:o.size] = rows[o], d[o]
    return lab, dist


def new_u8(dim):
    from longbow_amd import gpu
    return gpu.NewUint8Index(gpu.GPUConfig(DeviceID=0, Dimension=dim, Metric=0, DataType=gpu.DataType.Uint8))


def check(idx, Q, X, k, ctx):
    lab, dist = idx.SearchBatch(Q, k)
    D = ref_dist(Q, X)
    for q in range(Q.shape[0]):
        assert_same(lab[q], dist[q], *topk(D[q], k), f"{ctx} query {q}")
    assert idx._lib.lb_gpu_index_last_route(idx._h) == ROUTE_U8_SCAN


@pytest.mark.parametrize("data", ["uniform", "extremes"])
@pytest.mark.parametrize("nq", [1, 9, 40])
@pytest.mark.parametrize("dim", [16, 48, 100, 768])
def test_parity(dim, nq, data):
    gpu_or_skip()
    rng = np.random.default_rng(dim * 7 + nq)
    draw = (lambda *s: rng.integers(0, 256, s).astype(U8)) if data == "uniform" else (lambda *s: (rng.integers(0, 2, s) * 255).astype(U8))
    X, Q = draw(1000, dim), draw(nq, dim)
    with new_u8(dim) as idx:
        idx.Add(None, X)
        assert idx.dtype() == 3 and idx.ntotal == 1000
        check(idx, Q, X, 10, f"dim {dim} nq {nq} {data}")


# S far above 2^24 (rows 0..40 against queries 215..255 at D = 2048: S >= 2048 * 175^2): the chain arithmetic decides.  600 rows
# are one boot pass; 10,000 walk the classic schedule's admitting passes, 20,000 the sampled threshold and the striped lists,
# where the drop test runs.  mixed: half the rows lie near the queries, so both branches meet in one tile.
@pytest.mark.parametrize("kind,n,nq", [("far", 600, 1), ("far", 600, 20), ("far", 20000, 1), ("mixed", 600, 20), ("mixed", 10000, 1),
                                       ("mixed", 20000, 9)])
def test_slow_path(kind, n, nq):
    dim, k = 2048, 10
    rng = np.random.default_rng(n + nq)
    X = rng.integers(0, 41, (n, dim)).astype(U8)
    Q = rng.integers(215, 256, (nq, dim)).astype(U8)
    if kind == "mixed":
        near = Q[rng.integers(0, nq, n // 2)].astype(np.int64) + rng.integers(-40, 41, (n // 2, dim))
        X[1::2][:n // 2] = np.clip(near, 0, 255).astype(U8)
        k = n // 2 + 10 if n == 600 else k  # (a list that reaches into the far rows)
    if kind == "far":  # the test shows something only if sqrt(float32(S)) is not the answer
        d0 = ref_dist(Q[:1], X)[0]
        best = np.argsort(d0, kind="stable")[:k]
        S = ((X[best].astype(np.int64) - Q[0].astype(np.int64)) ** 2).sum(axis=1)
        assert S.min() > 1 << 24
        assert (d0[best] != np.sqrt(S.astype(F).astype(np.float64)).astype(F)).any()
    gpu_or_skip()
    with new_u8(dim) as idx:
        idx.Add(None, X)
        check(idx, Q, X, k, f"{kind} n {n} nq {nq}")


def test_ties_and_padding():
    gpu_or_skip()
    rng = np.random.default_rng(5)
    X = rng.integers(0, 256, (300, 16)).astype(U8)
    same = rng.choice(300, 64, replace=False)
    X[same] = X[same[0]]
    Q = np.stack([X[same[0]], rng.integers(0, 256, 16).astype(U8)])
    with new_u8(16) as idx:
        idx.Add(None, X)
        lab, _ = idx.SearchBatch(Q[:1], 64)
        assert lab[0].tolist() == sorted(same.tolist())  # ascending rows among equals
        check(idx, Q, X, 64, "ties")
        check(idx, Q, X, 310, "k > n")


def test_lifecycle_equals_a_fresh_index():
    gpu_or_skip()
    from longbow_amd import gpu
    rng = np.random.default_rng(11)
    n, dim, k = 5000, 48, 10
    X = rng.integers(0, 256, (n, dim)).astype(U8)
    Q = rng.integers(0, 256, (9, dim)).astype(U8)
    mask = (rng.random(n) < 0.1).astype(U8)
    vis = np.flatnonzero(mask)
    D = ref_dist(Q, X)
    want = [topk(D[q][vis], k, vis) for q in range(9)]
    with new_u8(dim) as idx, new_u8(dim) as fresh:
        idx.Add(None, X)
        fresh.Add(None, X[vis])
        flab, fdist = fresh.SearchBatch(Q, k)
        blab, bdist = idx.SearchBatch(Q, k, bitmap=gpu.pack_bitmap(mask)[0])  # the call's bitmap: a row list of 500 of 5,000
        idx.set_filter(mask)
        assert idx.nvisible() == vis.size
        mlab, mdist = idx.SearchBatch(Q, k)
        for q in range(9):
            assert_same(mlab[q], mdist[q], *want[q], f"set_filter query {q}")
            assert_same(blab[q], bdist[q], mlab[q], mdist[q], f"bitmap query {q}")
            assert_same(vis[flab[q]], fdist[q], mlab[q], mdist[q], f"fresh index query {q}")
        idx.set_filter(None)
        assert idx.remove_rows(np.flatnonzero(mask == 0)) == n - vis.size
        rlab, rdist = idx.SearchBatch(Q, k)
        assert np.array_equal(idx.Compact(), vis) and idx.ntotal == vis.size
        clab, cdist = idx.SearchBatch(Q, k)
        for q in range(9):
            assert_same(rlab[q], rdist[q], *want[q], f"removed query {q}")
            assert_same(clab[q], cdist[q], flab[q], fdist[q], f"compacted query {q}")


def test_wrong_element_type_refused_both_ways():
    lib = gpu_or_skip()
    from longbow_amd import gpu
    x = np.zeros(16, U8)
    out = (np.empty(1, F), np.empty(1, np.int64))
    with new_u8(16) as u8, gpu.NewIndexWithConfig(gpu.GPUConfig(Dimension=16, DataType=gpu.DataType.Int8)) as i8:
        for h, mine, add, search in [(u8, "uint8", lib.lb_gpu_index_add_i8, lib.lb_gpu_index_search_i8),
                                     (u8, "uint8", lib.lb_gpu_index_add, lib.lb_gpu_index_search),
                                     (i8, "int8", lib.lb_gpu_index_add_u8, lib.lb_gpu_index_search_u8)]:
            assert add(h._h, 1, x.ctypes.data, None) == 1
            assert f"holds {mine} rows" in lib.lb_gpu_last_error(h._h).decode()
            assert search(h._h, 1, x.ctypes.data, 1, out[0].ctypes.data, out[1].ctypes.data) == 1
            assert f"holds {mine} rows" in lib.lb_gpu_last_error(h._h).decode()
            assert h.ntotal == 0
        with pytest.raises(TypeError):
            u8.Add(None, x.astype(np.int8))
