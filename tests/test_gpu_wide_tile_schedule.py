"""The f32 wide tile's K-loop (gemm_filter_kernel<M, 2, 0>: strict mode, batches over 384 queries) against the oracle,
bit for bit: K-step counts 1, 2, 3 and 24 (the loop's peeled first, last-but-one and last steps), partial query and row
tiles, all three metrics, a row mask and a selective filter (compacted row list), the small-corpus bootstrap chunk, and
one full-size batch against the default mode.  D = 100 (D % 32 != 0, register-staged loop) is the control."""
import numpy as np
import pytest

from tests.gpu_util import assert_same, gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
WIDE = 4  # Index.last_route kind of the 128 x 128 f32 MFMA tile (gpu.Index.ROUTE_NAMES)


def _strict(d, metric, X, mask=None):
    idx = new_index(d, metric)
    idx.Add(None, X)
    idx.set_candidate_mode(0)  # strict: f32 MFMA candidates
    if mask is not None:
        idx.set_filter(mask)
    return idx


@pytest.mark.parametrize("d,n,nq", [
    (32, 300_001, 1061),   # nk = 1
    (64, 20_000, 385),     # nk = 2, small corpus: bootstrap chunk
    (96, 300_001, 385),    # nk = 3
    (768, 20_000, 1061),   # nk = 24
    (100, 20_000, 385),    # control: D % 32 != 0
])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_wide_tile_dims(oracle, d, n, nq, metric):
    gpu_or_skip()
    rng = np.random.default_rng(1000 + d + metric)
    X = rng.random((n, d), dtype=F)
    Q = rng.random((nq, d), dtype=F)
    k = 50
    idx = _strict(d, metric, X)
    lab, dist = idx.SearchBatch(Q, k)
    assert idx.last_route[0] == WIDE, idx.last_route
    assert idx.last_fallbacks == 0
    idx.Close()
    oi, od = oracle.search_batch(metric, Q, X, k, nthreads=16)
    assert_same(lab, dist, oi, od, f"d {d} n {n} nq {nq} metric {metric}")


@pytest.mark.parametrize("visible", [0.95, 0.02])  # per-row mask test / compacted row list
def test_wide_tile_filtered(oracle, visible):
    gpu_or_skip()
    rng = np.random.default_rng(77)
    n, d, nq, k = 300_001, 64, 385, 40
    X = rng.random((n, d), dtype=F)
    Q = rng.random((nq, d), dtype=F)
    mask = (rng.random(n) < visible).astype(np.uint8)
    for metric in (0, 1, 2):
        idx = _strict(d, metric, X, mask)
        lab, dist = idx.SearchBatch(Q, k)
        assert idx.last_route[0] == WIDE, idx.last_route
        assert idx.last_fallbacks == 0
        idx.Close()
        oi, od = oracle.search_batch(metric, Q, X, k, mask=mask, nthreads=16)
        assert_same(lab, dist, oi, od, f"visible {visible} metric {metric}")


def test_wide_tile_full_size_strict_equals_auto():
    """1024 x 1M x 768 cosine, k = 100: the strict mode (two wide-tile launches: sample and full pass) returns the
    default mode's lists for the whole batch"""
    gpu_or_skip()
    torch = pytest.importorskip("torch")
    from longbow_amd import _lib, gpu
    lib = _lib.load()
    N, D, B, K = 1_000_000, 768, 1024, 100
    X = torch.empty((N, D), device="cuda")
    Q = torch.empty((B, D), device="cuda")
    assert lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), X.numel(), 2024, 0, None) == 0
    assert lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), Q.numel(), 7, 0, None) == 0
    idx = gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=D, Metric=1))
    idx.reserve(N)
    idx.add_device(N, X.data_ptr())
    dist = torch.empty((B, K), device="cuda")
    lab = torch.empty((B, K), dtype=torch.int64, device="cuda")
    idx.search_device(B, Q.data_ptr(), K, dist.data_ptr(), lab.data_ptr())
    want = (lab.cpu().numpy(), dist.cpu().numpy())
    idx.set_candidate_mode(0)
    idx.search_device(B, Q.data_ptr(), K, dist.data_ptr(), lab.data_ptr())
    assert idx.last_route[0] == WIDE, idx.last_route
    assert idx.last_fallbacks == 0
    assert np.array_equal(lab.cpu().numpy(), want[0]) and np.array_equal(dist.cpu().numpy(), want[1])
    idx.Close()
