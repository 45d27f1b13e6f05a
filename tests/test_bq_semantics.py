"""Binary-quantisation semantics, no device needed: tests/bq_oracle.py against the reference tests' own literals
(tests/golden/bq_kats.json) and against hand-computed values."""
import math

import numpy as np
import pytest

from tests import bq_oracle as bo

F = np.float32


def test_oracle_reproduces_every_golden_case():
    enc, ham = bo.load_kats()
    assert len(enc) == 3 and len(ham) == 17
    for name, v, codes in enc:
        assert np.array_equal(bo.encode(v), codes), name
    for name, a, b, expected in ham:
        assert int(bo.hamming(a, b.reshape(1, -1))[0]) == expected, name


def test_encode_special_values():
    tiny = np.float32(1e-45)  # the smallest positive denormal
    assert tiny > 0 and tiny < np.finfo(F).tiny
    v = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, tiny, -tiny, np.finfo(F).tiny, -1.5, 2.5, np.finfo(F).max], F)
    want = [0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 1]
    code = bo.encode(v)
    assert code.shape == (1,)
    assert [(int(code[0]) >> i) & 1 for i in range(v.size)] == want
    assert int(code[0]) >> v.size == 0
    assert np.array_equal(bo.decode(code, v.size)[0], np.where(np.array(want) == 1, F(1), F(-1)))


@pytest.mark.parametrize("dims", [1, 63, 65, 100])
def test_pad_bits_are_zero(dims):
    codes = bo.encode(np.ones((3, dims), F))
    W = bo.words(dims)
    assert codes.shape == (3, W) and codes.dtype == np.uint64
    full = (1 << 64) - 1
    last = dims - 64 * (W - 1)
    for row in codes:
        assert all(int(w) == full for w in row[:-1])
        assert int(row[-1]) == (1 << last) - 1
    assert np.array_equal(bo.decode(codes, dims), np.ones((3, dims), F))


def test_distance_counts_whole_words():
    # pad bits a caller stored count, as in simd.HammingDistance: dims = 100, bit 127 set on one side
    a = np.array([0, 1 << 63], np.uint64)
    b = np.zeros((1, 2), np.uint64)
    assert int(bo.hamming(a, b)[0]) == 1


def test_topk_orders_by_distance_then_position_and_pads():
    d = np.array([5, 3, 5, 3, 9], np.int32)
    lab, dist = bo.topk(d, 3)
    assert lab.tolist() == [1, 3, 0] and dist.tolist() == [3.0, 3.0, 5.0]
    lab, dist = bo.topk(d, 7)
    assert lab.tolist() == [1, 3, 0, 2, 4, -1, -1]
    assert dist[5] == bo.FLT_MAX and dist[6] == bo.FLT_MAX and dist.dtype == F


def test_score_and_threshold_hand_computed():
    assert bo.score(0, 128) == F(1.0)
    assert bo.score(64, 128) == F(0.5)
    assert bo.score(128, 128) == F(0.0)
    assert bo.score(1, 3) == F(1.0) - F(1.0) / F(3.0)  # 0.6666666 as f32 operations
    assert bo.score(1, 3).dtype == F and float(bo.score(1, 3)) == 0.6666666269302368
    assert bo.score(np.array([0, 768]), 768).tolist() == [1.0, 0.0]
    assert bo.float32_to_hamming(1.0, 768) == 0
    assert bo.float32_to_hamming(0.5, 768) == 384
    assert bo.float32_to_hamming(0.0, 768) == 768
    assert bo.float32_to_hamming(0.75, 100) == 25
    # float32(0.9) = 0.89999998: 1000 * (1 - 0.89999998) = 100.00002 -> 100; float32(0.7) = 0.69999999: 10 * 0.30000001 -> 3
    assert bo.float32_to_hamming(0.9, 1000) == 100
    assert bo.float32_to_hamming(0.7, 10) == 3
    # float32(0.1) = 0.100000001: 10 * 0.899999999 = 8.99999999 -> 8 (the reference floors, it does not round)
    assert bo.float32_to_hamming(0.1, 10) == 8
    assert bo.float32_to_hamming(1.5, 64) == -32


def test_python_mirror_host_arithmetic_matches_the_oracle():
    from longbow_amd import bq
    enc = bq.BQEncoder.__new__(bq.BQEncoder)  # host arithmetic only: no handle
    enc._h = None
    for dims in (3, 64, 100, 768):
        enc.Dimensions = dims
        for h in (0, 1, dims // 2, dims):
            s = enc.ScoreToFloat32(h)
            assert s.dtype == F and s == bo.score(h, dims)
        for s in (0.0, 0.1, 0.5, 0.7, 0.9, 1.0):
            assert enc.Float32ToHamming(s) == bo.float32_to_hamming(s, dims)
            assert enc.Float32ToHamming(s) == int(math.floor(float(dims) * (1.0 - float(F(s)))))
