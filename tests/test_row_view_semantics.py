"""The oracle's predicate masks on the edge inputs of tests/row_view_cases.py, before the GPU is compared with it
(tests/test_gpu_row_views.py uses the same builders): every comparison operator over the int64 and float32 edge columns,
bitwise AndBytes, the Arrow validity rule at non-zero offsets, and the shapes of the structured masks themselves."""
import numpy as np
import pytest

from tests import row_view_cases as rc

F = np.float32


def test_int64_edge_column_all_ops(oracle):
    col = rc.int64_edge_column()
    assert col.size == 4099 and col.size % 16 != 0
    assert [int(v) for v in col[:16]] == list(rc.INT64_EDGES)  # nothing wrapped or saturated on the way into int64
    for val in rc.INT64_VALUES:
        for op in rc.OPS:
            got = oracle.match_int64(col, val, op)
            assert np.array_equal(got, rc.match_int64(col, val, op)), (val, op)
            # the first cycle once more with Python's unbounded integers: no fixed-width arithmetic at all
            py = [int((e == val, e != val, e > val, e >= val, e < val, e <= val)[op]) for e in rc.INT64_EDGES]
            assert list(got[:16]) == py, (val, op)


def test_int64_cases_tell_narrow_and_unsigned_compares_apart():
    """the column and values do catch the faults they are there for: a compare of the low words only, of the high words
    only, and an unsigned one each differ from the true result somewhere"""
    col = rc.int64_edge_column()

    def differs(view):
        return any(not np.array_equal(rc.match_int64(col, v, op), rc._compare(view(col), view(np.array([v], np.int64))[0], op))
                   for v in rc.INT64_VALUES for op in rc.OPS)

    assert differs(lambda a: a.astype(np.int32))                 # low 32 bits
    assert differs(lambda a: (a >> 32).astype(np.int32))         # high 32 bits
    assert differs(lambda a: a.view(np.uint64))                  # unsigned


def test_float32_edge_column_all_ops(oracle):
    col = rc.float32_edge_column()
    assert col.size == 4099
    bits = col[:16].view(np.uint32)
    assert bits[0] == 0x7FC00000 and bits[1] == 0xFFC00000       # NaN, -NaN
    assert bits[6] == 0x800116C2 and bits[10] == 0x000116C2      # -1e-40 / 1e-40: subnormal, not flushed on the way in
    assert bits[7] == 0x80000000 and bits[8] == 0 and bits[9] == 1  # -0, +0, the smallest subnormal
    for val in rc.FLOAT32_VALUES:
        for op in rc.OPS:
            got = oracle.match_float32(col, val, op)
            assert np.array_equal(got, rc.match_float32(col, val, op)), (val, op)
            with np.errstate(invalid="ignore"):
                assert np.array_equal(got, rc._compare(col, F(val), op).astype(np.uint8)), (val, op)  # numpy's own f32 compare


def test_float32_pinned_facts(oracle):
    col = rc.float32_edge_column(16)
    nan_rows = [0, 1]
    for val in rc.FLOAT32_VALUES:
        for op in rc.OPS:
            m = oracle.match_float32(col, val, op)
            assert list(m[nan_rows]) == [int(op == rc.NEQ)] * 2, (val, op)   # NaN != x is 1, every other op with NaN is 0
    for op in rc.OPS:                                                       # ... a NaN `value` included
        assert list(oracle.match_float32(col, np.nan, op)) == [int(op == rc.NEQ)] * 16
    neg0, pos0, tiny, sub = 7, 8, 9, 10
    for zero in (-0.0, 0.0):
        assert oracle.match_float32(col, zero, rc.EQ)[[neg0, pos0]].tolist() == [1, 1]   # -0 == +0
        assert oracle.match_float32(col, zero, rc.LT)[[neg0, pos0]].tolist() == [0, 0]
        assert oracle.match_float32(col, zero, rc.GT)[[tiny, sub]].tolist() == [1, 1]    # a subnormal is > 0 ...
        assert oracle.match_float32(col, zero, rc.NEQ)[[tiny, sub]].tolist() == [1, 1]   # ... and != 0
        assert oracle.match_float32(col, zero, rc.LT)[6] == 1                            # -1e-40 < 0
    assert oracle.match_float32(col, 1e-40, rc.EQ).tolist() == [int(i == sub) for i in range(16)]
    assert oracle.match_float32(col, 1e-40, rc.GT)[[tiny, sub, 11]].tolist() == [0, 0, 1]


def test_second_round_columns(oracle):
    """the large columns put their distinguishing values where the second round of match_kernel's loop works"""
    assert rc.MATCH_ROUND == 16_777_216 and rc.AND_ROUND == 1_048_576 and rc.BIG_N == 16_777_216 + 48 + 5
    second = [p for p in rc.BIG_POSITIONS if p >= rc.MATCH_ROUND]
    assert any((p - rc.MATCH_ROUND) // 16 < 3 for p in second) and any((p - rc.MATCH_ROUND) // 16 == 3 for p in second)
    assert max(second) == rc.BIG_N - 1
    lo = rc.MATCH_ROUND - 64
    for col, val, ref, oref in ((rc.big_int64_column(), rc.BIG_INT64_VALUE, rc.match_int64, oracle.match_int64),
                                (rc.big_float32_column(), rc.BIG_FLOAT32_VALUE, rc.match_float32, oracle.match_float32)):
        for op in (rc.EQ, rc.LT):
            got = oref(col, val, op)
            assert np.array_equal(got[lo:], ref(col[lo:], val, op))
            marks = np.zeros(col.size, bool)
            marks[list(rc.BIG_POSITIONS)] = True
            # the constant part is all 1 (EQ) or all 0 (LT); the marks differ from it under EQ and split under LT
            assert np.all(got[~marks] == (1 if op == rc.EQ else 0))
            assert not got[marks].any() if op == rc.EQ else 0 < got[marks].sum() < marks.sum()


def test_and_bytes_is_bitwise(oracle):
    rng = np.random.default_rng(11)
    for n in (1, 255, 256, 257, 5000):
        a = rng.integers(0, 256, n).astype(np.uint8)
        b = rng.integers(0, 256, n).astype(np.uint8)
        assert np.array_equal(oracle.and_bytes(a, b), rc.and_bytes(a, b))
    assert oracle.and_bytes(np.array([2, 0x80, 0xFF, 3], np.uint8), np.array([1, 0xFF, 0x81, 6], np.uint8)).tolist() == [0, 0x80, 0x81, 2]


@pytest.mark.parametrize("offset", [0, 1, 7, 8, 13, 67])
def test_validity_rule_and_bitmap_builder(offset):
    rng = np.random.default_rng(offset)
    for n in (1, 8, 1999, 2000, 2001, 2047, 2049):
        valid = rng.random(n) > 0.3
        bm = rc.validity_bitmap(valid, offset)
        assert bm.size == (offset + n + 7) // 8                    # exactly the bytes filter_column uploads
        got = rc.validity(bm, offset, n)
        assert np.array_equal(got, valid.astype(np.uint8))
        assert got.tolist() == [(int(bm[(i + offset) >> 3]) >> ((i + offset) & 7)) & 1 for i in range(n)]
        assert np.array_equal(got, np.unpackbits(bm, bitorder="little")[offset:offset + n])
        bits = np.unpackbits(bm, bitorder="little")
        if offset:
            assert bits[offset - 1] != valid[0]                    # reading one bit early shows
        if bits.size > offset + n:
            assert bits[offset + n] != valid[-1]                   # one bit late as well


def test_predicate_is_match_and_validity(oracle):
    rng = np.random.default_rng(5)
    col = rng.permutation(rc.int64_edge_column(2001))
    valid = rng.random(2001) > 0.2
    exp = rc.predicate(col, 2 ** 32 + 5, rc.LT, valid)
    assert np.array_equal(exp, oracle.and_bytes(oracle.match_int64(col, 2 ** 32 + 5, rc.LT), valid.astype(np.uint8)))
    assert not exp[~valid].any()                                   # nulls never match


def test_mask_builders():
    rng = np.random.default_rng(7)
    n, k = 20000, 10
    masks = rc.structured_masks(n, k, rng)
    assert np.flatnonzero(masks["row 0"]).tolist() == [0] and np.flatnonzero(masks["row n-1"]).tolist() == [n - 1]
    vis = np.flatnonzero(masks["last partial block"])
    assert vis[0] == 18432 and vis[-1] == n - 1 and vis.size == n - 18432 and vis.size < rc.CP_ROWS
    for c in (k - 1, k, k + 1):
        m = masks[f"{c} rows spread"]
        assert m.sum() == c and m[0] and m[n - 1]
    per_block = np.add.reduceat(masks["one row per block"], np.arange(0, n, rc.CP_ROWS))
    assert per_block.tolist() == [1] * 10
    assert masks["all but one"].sum() == n - 1
    # the list / mask switch: equality takes the list
    for nn, lo in ((2000, 1900), (20000, 19000)):
        assert rc.takes_row_list(lo, nn) and not rc.takes_row_list(lo + 1, nn)
        assert rc.exact_count_mask(rng, nn, lo).sum() == lo
    for frac in (0.5, 0.98):
        m = rc.byte_mask(rng, n, frac)
        assert set(np.unique(m).tolist()) == set(rc.MASK_BYTES)
        assert rc.takes_row_list(int((m != 0).sum()), n) == (frac == 0.5)
