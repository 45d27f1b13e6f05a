"""What a search under a row bitmap given with the call means on the flat index (include/longbow_gpu.h, lb_gpu_index_*: "call
bitmap"), pinned on the CPU: the expected-result helper of tests/index_bitmap_cases.py is the oracle's search over the rows whose
bit is set (and that the handle's own mask leaves), bits at or past nbits change nothing, the packing round-trips at the sizes where
a byte or a block ends, and gpu.pack_bitmap is the very function ivf.pack_bitmap is.  tests/test_gpu_index_bitmap.py compares the
library with the same helper on the same shapes."""
import numpy as np
import pytest

from tests import index_bitmap_cases as ic
from tests import ivf_bitmap_cases as bc
from tests import row_view_cases as rc

F = np.float32
FLT_MAX = np.finfo(F).max


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(7)
    n, d = 300, 12
    return rng.random((n, d), dtype=F), rng.random((5, d), dtype=F), rng


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_helper_is_the_oracle_over_the_rows_whose_bit_is_set(oracle, data, metric):
    X, Q, _ = data
    n, k = X.shape[0], 10
    rng = np.random.default_rng(metric)
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    also = rng.choice(np.array(rc.MASK_BYTES, np.uint8), n)            # a handle filter's bytes: visible iff non-zero
    lab, dist = ic.search_bitmap(oracle, metric, Q, X, k, bc.pack(mask), also=also)
    vis = np.flatnonzero((mask != 0) & (also != 0))
    assert 0 < vis.size < mask.sum()
    for q in range(Q.shape[0]):                                         # restated: the visible rows alone, canonical order
        d = oracle.batch_flat(metric, Q[q], X[vis])
        oi, od, _ = oracle.topk_canonical(d, k)
        assert np.array_equal(lab[q], vis[oi]) and np.array_equal(dist[q], od)
    # ids: labels are ids[row]
    ids = (np.arange(n, dtype=np.int64) * 7 + 1000)
    lab2, dist2 = ic.search_bitmap(oracle, metric, Q, X, k, bc.pack(mask), also=also, ids=ids)
    assert np.array_equal(lab2, ids[lab]) and np.array_equal(dist2, dist)


def test_fewer_than_k_rows_pad(oracle, data):
    X, Q, _ = data
    mask = np.zeros(X.shape[0], np.uint8)
    mask[[3, 299]] = 1
    lab, dist = ic.search_bitmap(oracle, 0, Q, X, 5, bc.pack(mask))
    assert np.all(np.sort(lab[:, :2], axis=1) == [3, 299]) and np.all(lab[:, 2:] == -1) and np.all(dist[:, 2:] == FLT_MAX)
    lab, dist = ic.search_bitmap(oracle, 0, Q, X, 5, bc.pack(np.zeros(X.shape[0], np.uint8)))
    assert np.all(lab == -1) and np.all(dist == FLT_MAX)


@pytest.mark.parametrize("n", [1, 7, 9, 13, 299])
def test_bits_at_or_past_nbits_change_nothing(oracle, data, n):
    X, Q, _ = data
    rng = np.random.default_rng(n)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    mask[0] = 1
    bits = bc.pack(mask)
    tail = ic.with_tail_ones(bits, n)
    assert n % 8 == 0 or not np.array_equal(bits, tail)
    assert np.array_equal(ic.effective_mask(tail, n), mask)
    longer = np.concatenate([tail, np.full(3, 0xFF, np.uint8)])         # and bytes behind the last one
    assert np.array_equal(ic.effective_mask(longer, n), mask)
    a = ic.search_bitmap(oracle, 0, Q, X[:n], 4, bits)
    b = ic.search_bitmap(oracle, 0, Q, X[:n], 4, longer)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("n", ic.ROUND_TRIP_N)
def test_pack_unpack_round_trip(n):
    from longbow_amd import gpu
    rng = np.random.default_rng(n)
    for mask in (np.zeros(n, np.uint8), np.ones(n, np.uint8), (rng.random(n) < 0.5).astype(np.uint8),
                 rng.choice(np.array(rc.MASK_BYTES, np.uint8), n)):
        bits, stride = gpu.pack_bitmap(mask)
        assert stride == 0 and bits.dtype == np.uint8 and bits.shape == (bc.nbytes(n),)
        assert np.array_equal(bits, bc.pack(mask))                       # bit by bit, padding bits zero
        assert np.array_equal(bc.unpack(bits, n), (mask != 0).astype(np.uint8))
        assert np.array_equal(gpu.pack_bitmap(mask != 0)[0], bits)      # a bool mask too


def test_pack_bitmap_is_one_function():
    from longbow_amd import _rowfilter, gpu, ivf
    assert gpu.pack_bitmap is ivf.pack_bitmap is _rowfilter.pack_bitmap


def test_shapes_cover_the_edges():
    assert ic.BLOCK == 2048 and set(ic.ROUND_TRIP_N) <= set(ic.EDGE_N)
    n = 20000
    counts = ic.view_edge_counts(n)
    assert [c for c, _ in counts] == [18999, 19000, 19001, 19999]
    assert [lst for _, lst in counts] == [True, True, False, False]     # both forms of the view run
    m = ic.block_gap_mask(3 * ic.BLOCK + 5, np.random.default_rng(0))
    per_block = [int(m[b:b + ic.BLOCK].sum()) for b in range(0, m.size, ic.BLOCK)]
    assert per_block[0] > 0 and per_block[1] == per_block[2] == 0 and per_block[3] > 0
