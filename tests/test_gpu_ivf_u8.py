"""lb_gpu_ivf_new_u8 on the GPU.  Expected: distances from tests/test_gpu_u8.py's float32 numpy restatement of the reference's four
chains, lists and probes from tests/ivf_oracle.py over the widened rows and queries, the canonical top-k over the probed rows."""
import numpy as np
import pytest

from tests import ivf_oracle as io
from tests.gpu_util import assert_same, gpu_or_skip
from tests.test_gpu_u8 import new_u8, ref_dist, topk

pytestmark = pytest.mark.gpu
F, U8 = np.float32, np.uint8
TILE, EXACT = 128, 1 << 24  # rows per tile of the staged scan; the largest sum whose f32 adds are all exact


def _u8(X, C_):
    from longbow_amd import ivf
    gpu_or_skip()
    h = ivf.IVFFlatUint8(C_)
    if X.shape[0]:
        h.add(X)
    return h


def _draw(rng, data, *shape):
    return rng.integers(0, 256, shape).astype(U8) if data == "uniform" else (rng.integers(0, 2, shape) * 255).astype(U8)


def _want(oracle, Q, X, C_, lists, k, nprobe, D=None):
    D = ref_dist(Q, X) if D is None else D  # (where the caller has it already)
    out = [topk(D[j, rows], k, rows) for j in range(Q.shape[0])
           for rows in [io.probed_rows(lists, io.probes(oracle, 0, 0, Q[j].astype(F), C_, nprobe))]]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _chains(Q, X):
    # -> [4, nq, n] int64: the exact sum of chain j of every pair (D % 4 == 0); the per-chain formula's value of every pair
    d = X.astype(np.int64)[None, :, :] - Q.astype(np.int64)[:, None, :]
    S = np.stack([(d[:, :, j::4] ** 2).sum(axis=2) for j in range(4)])
    s = S.astype(F)
    return S, np.sqrt((((s[0] + s[1]) + s[2]) + s[3]).astype(np.float64)).astype(F)


# 16 one piece; 128 totals form, half a stage; 256 a full stage; 272 the smallest multiple of 16 above 258: chains form, a
# partial second stage; 768 three stages; 1040 above 1032; 20, 100 the generic form
@pytest.mark.parametrize("data", ["uniform", "extremes"])
@pytest.mark.parametrize("dim", [16, 128, 256, 272, 768, 1040, 20, 100])
def test_dimensions_and_forms(oracle, dim, data):
    rng = np.random.default_rng(dim * 3 + len(data))
    n, nlist = 1000, 6
    X, Q9 = _draw(rng, data, n, dim), _draw(rng, data, 9, dim)
    C_ = X[np.sort(rng.permutation(n)[:nlist])].astype(F) + rng.standard_normal((nlist, dim)).astype(F)  # (no two alike)
    lists, D9 = io.assign(oracle, 0, 0, X.astype(F), C_), ref_dist(Q9, X)
    h = _u8(X, C_)
    assert h.dtype == 3 and h.ntotal == n and np.array_equal(h.assignments(), lists)
    with new_u8(dim) as flat:
        flat.Add(None, X)
        for nq in (1, 9):
            Q, D = Q9[:nq], D9[:nq]
            for nprobe in (1, 2, nlist):
                assert_same(*h.search(Q, 10, nprobe), *_want(oracle, Q, X, C_, lists, 10, nprobe, D), f"nq {nq} nprobe {nprobe}")
            assert_same(*h.search(Q, 10, nlist), *flat.SearchBatch(Q, 10), f"flat uint8 index, nq {nq}")
    h.Close()


@pytest.mark.parametrize("dim", [768, 1040])
def test_the_per_chain_path_decides(oracle, dim):
    # 0/255 bytes: every pair beyond 2^24 in total, no chain beyond it; sqrt(float32(S)) is not the reference's value
    rng = np.random.default_rng(dim)
    n, nlist = 500, 4
    X, Q = _draw(rng, "extremes", n, dim), _draw(rng, "extremes", 4, dim)
    (S, per_chain), D = _chains(Q, X), ref_dist(Q, X)
    assert S.sum(axis=0).min() > EXACT and S.max() <= EXACT and np.array_equal(per_chain, D)
    differs = D != np.sqrt(S.sum(axis=0).astype(F).astype(np.float64)).astype(F)
    print(f"dim {dim}: sqrt(float32(S)) differs from the reference in {differs.sum()} of {differs.size} pairs")
    assert differs.any()
    C_ = X[:nlist].astype(F) + rng.standard_normal((nlist, dim)).astype(F)
    lists = io.assign(oracle, 0, 0, X.astype(F), C_)
    h = _u8(X, C_)
    for nprobe in (2, nlist):  # k = n: every probed row is returned
        assert_same(*h.search(Q, n, nprobe), *_want(oracle, Q, X, C_, lists, n, nprobe, D), f"nprobe {nprobe}")
    h.Close()


@pytest.mark.parametrize("kind", ["far", "mixed"])
def test_the_chain_fallback_decides(oracle, kind):
    # rows in 0..20 against queries in 235..255 at D = 2048: every chain beyond 2^24, the chain arithmetic from memory decides;
    # mixed: half the rows lie near the queries, so both branches meet in one tile
    rng = np.random.default_rng(len(kind))
    n, nlist, dim = 600, 4, 2048
    X, Q = rng.integers(0, 21, (n, dim)).astype(U8), rng.integers(235, 256, (9, dim)).astype(U8)
    far = np.ones(n, bool)
    if kind == "mixed":
        far[1::2] = False
        X[1::2] = np.clip(Q[rng.integers(0, 9, n // 2)].astype(np.int64) + rng.integers(-40, 41, (n // 2, dim)), 0, 255).astype(U8)
    (S, per_chain), D = _chains(Q, X), ref_dist(Q, X)
    print(f"{kind}: the smallest chain sum of a far pair is {S[:, :, far].min()}")
    assert S[:, :, far].min() > EXACT and (per_chain[:, far] != D[:, far]).any()
    # 128 +- 1 with as many of either sign: a row's list follows its own noise, so near and far rows share the lists
    C_ = np.stack([128 + rng.permutation(np.repeat([-1.0, 1.0], dim // 2)) for _ in range(nlist)]).astype(F)
    lists = io.assign(oracle, 0, 0, X.astype(F), C_)
    assert kind == "far" or all(0 < far[lists == l].mean() < 1 for l in range(nlist))
    h = _u8(X, C_)
    for nprobe in (2, nlist):
        assert_same(*h.search(Q, n, nprobe), *_want(oracle, Q, X, C_, lists, n, nprobe, D), f"{kind} nprobe {nprobe}")
    h.Close()


def test_list_length_edges_and_a_misaligned_base(oracle):
    import torch
    counts = (0, 1, TILE - 1, TILE, TILE + 1)
    Xf, Qf, C_, owner = io.edge_case(counts, dim=16, noise=1.0)
    X, Q = np.clip(np.rint(Xf), 0, 255).astype(U8), np.clip(np.rint(Qf), 0, 255).astype(U8)
    assert np.array_equal(io.assign(oracle, 0, 0, X.astype(F), C_), owner)
    h, D = _u8(X, C_), ref_dist(Q, X)
    assert h.list_sizes().tolist() == list(counts)
    for nprobe, k in ((1, 10), (1, 200), (5, 10), (5, 200)):
        assert_same(*h.search(Q, k, nprobe), *_want(oracle, Q, X, C_, owner, k, nprobe, D), f"nprobe {nprobe} k {k}")
    lab, dist = h.search(Q, 10, 1)
    assert (lab[0] == -1).all() and (dist[0] == io.FLT_MAX).all()  # an empty probed list: all padding
    nq, k = Q.shape[0], 40  # queries at an odd byte address take the one-lane-per-row form
    buf = torch.zeros(Q.size + 16, dtype=torch.uint8, device="cuda")
    buf[1:1 + Q.size] = torch.from_numpy(Q).cuda().reshape(-1)
    dD, dL = torch.full((nq, k), -5.0, device="cuda"), torch.full((nq, k), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0 and dD.dtype == torch.float32
    h.search_device(nq, buf.data_ptr() + 1, k, 2, dD.data_ptr(), dL.data_ptr())
    assert_same(dL.cpu().numpy(), dD.cpu().numpy(), *_want(oracle, Q, X, C_, owner, k, 2, D), "queries at 1 mod 16")
    h.Close()


def test_one_workgroup_walks_several_tiles_and_stages(oracle):
    # 128 queries x 32 probes = 4,096 pairs: one workgroup per (query, list) walks the three or more tiles of a list, three stages
    # each (528 dims, the chains form), wrapping from a tile's last stage to the next tile's first
    rng = np.random.default_rng(528)
    n, dim, nlist = 16000, 528, 40
    X, Q = _draw(rng, "uniform", n, dim), _draw(rng, "uniform", 128, dim)
    C_ = X[np.sort(rng.permutation(n)[:nlist])].astype(F)
    lists = io.assign(oracle, 0, 0, X.astype(F), C_)
    sizes = np.bincount(lists, minlength=nlist)
    assert np.median(sizes) > 2 * TILE and sizes.max() > 3 * TILE, sizes
    h = _u8(X, C_)
    assert_same(*h.search(Q, 10, 32), *_want(oracle, Q, X, C_, lists, 10, 32), "several tiles and stages")
    h.Close()


def test_lifecycle_equals_a_fresh_handle():
    from longbow_amd import ivf
    rng = np.random.default_rng(11)
    n, dim, k, nlist, nprobe = 5000, 48, 10, 8, 3
    X, Q = _draw(rng, "uniform", n, dim), _draw(rng, "uniform", 9, dim)
    C_, mask = X[:nlist].astype(F), (rng.random(n) < 0.1).astype(U8)
    vis = np.flatnonzero(mask)
    h, fresh, wide = _u8(X, C_), _u8(X[vis], C_), ivf.IVFFlat(C_)
    wide.add(X.astype(F))
    assert np.array_equal(h.assignments(), wide.assignments()) and np.array_equal(h.list_sizes(), wide.list_sizes())
    flab, fdist = fresh.search(Q, k, nprobe)
    assert (flab >= 0).all()
    assert_same(*h.search(Q, k, nprobe, bitmap=ivf.pack_bitmap(mask)[0]), vis[flab], fdist, "call bitmap")
    h.set_filter(mask)
    assert h.nvisible() == vis.size
    assert_same(*h.search(Q, k, nprobe), vis[flab], fdist, "set_filter")
    h.set_filter(None)
    assert h.remove_rows(np.flatnonzero(mask == 0)) == n - vis.size
    assert_same(*h.search(Q, k, nprobe), vis[flab], fdist, "remove_rows")
    assert np.array_equal(h.compact(), vis) and h.ntotal == vis.size
    assert_same(*h.search(Q, k, nprobe), flab, fdist, "compact")
    for x in (h, fresh, wide):
        x.Close()


def test_wrong_element_type_refused_both_ways():
    from longbow_amd import ivf
    lib = gpu_or_skip()
    C_, x = np.eye(4, 16, dtype=F), np.zeros(16, U8)
    dist, lab = np.full(1, 9.0, F), np.full(1, 77, np.int64)
    u8, i8, f32 = _u8(np.zeros((0, 16), U8), C_), ivf.IVFFlatInt8(C_), ivf.IVFFlat(C_)
    for h, mine, add, search in [(u8, "uint8", lib.lb_gpu_ivf_add_i8, lib.lb_gpu_ivf_search_i8),
                                 (u8, "uint8", lib.lb_gpu_ivf_add, lib.lb_gpu_ivf_search),
                                 (i8, "int8", lib.lb_gpu_ivf_add_u8, lib.lb_gpu_ivf_search_u8),
                                 (f32, "float32", lib.lb_gpu_ivf_add_u8, lib.lb_gpu_ivf_search_u8)]:
        assert add(h._h, 1, x.ctypes.data, None) == 1
        assert f"holds {mine} rows" in lib.lb_gpu_ivf_last_error(h._h).decode()
        assert search(h._h, 1, x.ctypes.data, 1, 1, dist.ctypes.data, lab.ctypes.data) == 1
        assert f"holds {mine} rows" in lib.lb_gpu_ivf_last_error(h._h).decode()
        assert h.ntotal == 0 and dist[0] == 9.0 and lab[0] == 77
    for h in (u8, i8, f32):
        h.Close()
