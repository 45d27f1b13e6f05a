"""uint8 index, i8 matrix-core pass (route 83): labels and distance bits equal to the numpy restatement of the reference's
euclideanUint8Unrolled4x in tests/test_gpu_u8.py, at the shapes where the pass's staging, padding and epilogue can go wrong."""
import numpy as np
import pytest

from tests.gpu_util import assert_same, gpu_or_skip
from tests.test_gpu_u8 import F, U8, new_u8, ref_dist, topk

pytestmark = pytest.mark.gpu

ROUTE_U8_SCAN, ROUTE_U8_MFMA = 82, 83
N_PARITY = 128 * 128 + 77  # the last tile is partial


def draw(rng, data, *shape):
    return rng.integers(0, 256, shape).astype(U8) if data == "uniform" else (rng.integers(0, 2, shape) * 255).astype(U8)


def check(idx, Q, X, k, route, ctx, vis=None, relabel=None, **kw):
    """the search against top-k of the reference values over the rows `vis` (all); relabel: old row of each reported label"""
    lab, dist = idx.SearchBatch(Q, k, **kw)
    assert idx._lib.lb_gpu_index_last_route(idx._h) == route, ctx
    D = ref_dist(Q, X) if isinstance(X, np.ndarray) else X[0]
    for q in range(Q.shape[0]):
        want = topk(D[q], k) if vis is None else topk(D[q][vis], k, vis)
        got = lab[q] if relabel is None else np.where(lab[q] >= 0, relabel[np.maximum(lab[q], 0)], -1)
        assert_same(got, dist[q], *want, f"{ctx} query {q}")


# (dim, nq): one padded stage / a second query tile of one query; one exactly full stage; a full plus a partial stage; a partial
# 32-column block; six stages.  extremes: -128 * -128 and the sign of the shift
@pytest.mark.parametrize("dim,nq,k,data", [(d, q, 10, data) for d, q in [(16, 16), (16, 129), (128, 33), (144, 129), (768, 33)]
                                           for data in ("uniform", "extremes")] + [(144, 33, 1, "uniform"), (144, 33, 100, "uniform")])
def test_parity(dim, nq, k, data):
    gpu_or_skip()
    rng = np.random.default_rng(dim * 7 + nq + k)
    X, Q = draw(rng, data, N_PARITY, dim), draw(rng, data, nq, dim)
    with new_u8(dim) as idx:
        idx.Add(None, X)
        check(idx, Q, X, k, ROUTE_U8_MFMA, f"dim {dim} nq {nq} k {k} {data}")


# S far above 2^24 (test_gpu_u8.test_slow_path's constructions): far -- the sample pass recomputes every pair, the admitting pass
# drops by the lower bound and recomputes what it admits; mixed -- both branches inside one 32 x 32 block
@pytest.mark.parametrize("kind", ["far", "mixed"])
def test_beyond_2_24(kind):
    dim, n, nq, k = 2048, 20000, 20, 10
    rng = np.random.default_rng(n + nq)
    X = rng.integers(0, 41, (n, dim)).astype(U8)
    Q = rng.integers(215, 256, (nq, dim)).astype(U8)
    if kind == "mixed":
        near = Q[rng.integers(0, nq, n // 2)].astype(np.int64) + rng.integers(-40, 41, (n // 2, dim))
        X[1::2][:n // 2] = np.clip(near, 0, 255).astype(U8)
    D = ref_dist(Q, X)
    if kind == "far":  # the test shows something only if sqrt(float32(S)) is not the answer
        best = np.argsort(D[0], kind="stable")[:k]
        S = ((X[best].astype(np.int64) - Q[0].astype(np.int64)) ** 2).sum(axis=1)
        assert S.min() > 1 << 24
        assert (D[0][best] != np.sqrt(S.astype(F).astype(np.float64)).astype(F)).any()
    gpu_or_skip()
    with new_u8(dim) as idx:
        idx.Add(None, X)
        check(idx, Q, (D,), k, ROUTE_U8_MFMA, kind)


@pytest.fixture(scope="module")
def view_corpus():
    rng = np.random.default_rng(48)
    X, Q = draw(rng, "uniform", 40000, 48), draw(rng, "uniform", 33, 48)
    return X, Q, (ref_dist(Q, X),), (rng.random(40000) < 0.5).astype(U8), (rng.random(40000) < 0.97).astype(U8)


# hidden rows reach the kernel as a row list (50 % visible), as the per-row mask test (97 %), through the call's bitmap, as
# tombstones and, after Compact, not at all; 20,000 visible rows stay above the sample floor
@pytest.mark.parametrize("view", ["filter50", "filter97", "bitmap50", "remove50"])
def test_row_views(view_corpus, view):
    gpu_or_skip()
    from longbow_amd import gpu
    X, Q, D, half, most = view_corpus
    mask = most if view == "filter97" else half
    vis = np.flatnonzero(mask)
    with new_u8(48) as idx:
        idx.Add(None, X)
        if view == "bitmap50":
            check(idx, Q, D, 10, ROUTE_U8_MFMA, view, vis, bitmap=gpu.pack_bitmap(mask)[0])
        elif view == "remove50":
            assert idx.remove_rows(np.flatnonzero(mask == 0)) == X.shape[0] - vis.size
            check(idx, Q, D, 10, ROUTE_U8_MFMA, "removed", vis)
            assert np.array_equal(idx.Compact(), vis)
            check(idx, Q, D, 10, ROUTE_U8_MFMA, "compacted", vis, relabel=vis)
        else:
            idx.set_filter(mask)
            check(idx, Q, D, 10, ROUTE_U8_MFMA, view, vis)


# below LB_U8_MFMA_MINQ queries, or at a dimension that is no multiple of 16, the scan serves the batch as before
@pytest.mark.parametrize("dim,nq", [(144, 15), (100, 33)])
def test_gate_keeps_the_scan(dim, nq):
    gpu_or_skip()
    rng = np.random.default_rng(144 * 7 + 33)
    X, Q = draw(rng, "uniform", N_PARITY, 144)[:, :dim].copy(), draw(rng, "uniform", nq, 144)[:, :dim].copy()
    with new_u8(dim) as idx:
        idx.Add(None, X)
        check(idx, Q, X, 10, ROUTE_U8_SCAN, f"dim {dim} nq {nq}")
