"""The 256-row body of the f32 wide tile (gemm_filter_wide256_kernel: 256 rows x 128 queries on a three-stage ring of 16-k
stages) against the oracle, bit for bit, in strict mode on the diagnostic library with the body's minimum tile count lowered
(lb_debug_set_wide256_min_tiles), so that small shapes reach it: K-step counts 2, 4, 6 and 48 (the loop's three peeled
steps), partial row tiles on both sides of the 128-row half, partial and full query tiles, all three metrics, a row mask and
a compacted row list.  D = 48 (D % 32 != 0) and a pass with too few tiles at the default minimum stay on the 128-row tile."""
import functools

import numpy as np
import pytest

from tests.gpu_util import assert_same, diag_lib, new_index

pytestmark = pytest.mark.gpu
F = np.float32
WIDE = 4  # Index.last_route kind of the f32 MFMA tile (gpu.Index.ROUTE_NAMES)


@pytest.fixture
def lib():
    lib = diag_lib()
    yield lib
    lib.lb_debug_set_wide256_min_tiles(-1)  # back to the compiled-in minimum


@functools.lru_cache(maxsize=None)
def _data(d, n, nq, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d), dtype=F)
    Q = rng.random((nq, d), dtype=F)
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


_refs = {}


def _reference(oracle, metric, d, n, nq, seed, k, mask=None, mask_key=None):
    key = (metric, d, n, nq, seed, k, mask_key)
    if key not in _refs:
        X, Q = _data(d, n, nq, seed)
        _refs[key] = oracle.search_batch(metric, Q, X, k, mask=mask, nthreads=16) if mask is not None else \
            oracle.search_batch(metric, Q, X, k, nthreads=16)
    return _refs[key]


def _search(lib, d, metric, X, Q, k, min_tiles, mask=None):
    """strict-mode search on the diagnostic library; returns (labels, distances, rows of the last non-boot wide launch)"""
    idx = new_index(d, metric, lib=lib)
    idx.Add(None, X)
    idx.set_candidate_mode(0)  # strict: f32 MFMA candidates
    if mask is not None:
        idx.set_filter(mask)
    lib.lb_debug_set_wide256_min_tiles(min_tiles)  # (also forgets the last launch's tile)
    lab, dist = idx.SearchBatch(Q, k)
    assert idx.last_route[0] == WIDE, idx.last_route
    assert idx.last_fallbacks == 0
    rows = lib.lb_debug_last_wide_rows()
    idx.Close()
    return lab, dist, rows


@pytest.mark.parametrize("d,n,nq,rows", [
    (32, 300_001, 1061, 256),  # 2 K-steps: the last two peeled steps only
    (48, 300_001, 385, 128),   # D % 32 != 0: stays on the 128-row tile
    (64, 300_001, 385, 256),   # 4 K-steps: one full step, then the three peeled ones
    (96, 300_001, 385, 256),   # 6 K-steps
    (768, 20_000, 513, 256),   # 48 K-steps
])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_wide256_ring_edges(oracle, lib, d, n, nq, rows, metric):
    k = 50
    X, Q = _data(d, n, nq, 2000 + d)
    lab, dist, got_rows = _search(lib, d, metric, X, Q, k, 1)
    assert got_rows == rows
    oi, od = _reference(oracle, metric, d, n, nq, 2000 + d, k)
    assert_same(lab, dist, oi, od, f"d {d} n {n} nq {nq} metric {metric}")


# n mod 256 in {1, 127, 129, 255}, row-tile counts 65, 65, 65, 68 (no multiple of 8: the XCD order's last group is partial);
# 385 queries: the last query tile holds one query; 512: full query tiles only
@pytest.mark.parametrize("n,nq", [(16_385, 385), (16_511, 385), (16_513, 385), (16_639 + 256 * 3, 385), (16_385, 512)])
def test_wide256_row_and_query_edges(oracle, lib, n, nq):
    d, k = 64, 50
    X, Q = _data(d, n, nq, 31)
    for metric in (0, 1, 2):
        lab, dist, rows = _search(lib, d, metric, X, Q, k, 1)
        assert rows == 256
        oi, od = _reference(oracle, metric, d, n, nq, 31, k)
        assert_same(lab, dist, oi, od, f"n {n} nq {nq} metric {metric}")


@pytest.mark.parametrize("visible", [0.95, 0.02])  # per-row mask test / compacted row list
def test_wide256_filtered(oracle, lib, visible):
    d, n, nq, k = 64, 300_001, 385, 40
    X, Q = _data(d, n, nq, 2000 + d)
    mask = (np.random.default_rng(78).random(n) < visible).astype(np.uint8)
    for metric in (0, 1, 2):
        lab, dist, rows = _search(lib, d, metric, X, Q, k, 1, mask=mask)
        assert rows == 256
        oi, od = _reference(oracle, metric, d, n, nq, 2000 + d, k, mask=mask, mask_key=visible)
        assert_same(lab, dist, oi, od, f"visible {visible} metric {metric}")


def test_wide256_default_minimum_keeps_small_passes_on_128(oracle, lib):
    """control: 68 x 4 tiles of 256 rows are fewer than the compiled-in minimum -- the 128-row tile, the same lists"""
    d, n, nq, k = 64, 16_639 + 256 * 3, 385, 50
    X, Q = _data(d, n, nq, 31)
    for metric in (0, 1, 2):
        lab, dist, rows = _search(lib, d, metric, X, Q, k, -1)
        assert rows == 128
        oi, od = _reference(oracle, metric, d, n, nq, 31, k)
        assert_same(lab, dist, oi, od, f"control metric {metric}")
