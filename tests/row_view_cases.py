"""Inputs and plain numpy restatements shared by tests/test_row_view_semantics.py (CPU: the oracle is pinned on them)
and tests/test_gpu_row_views.py (GPU: the kernels are compared with the oracle on exactly the same inputs).

Restated here, independently of oracle/longbow_oracle.c:
- simd.MatchInt64 / simd.MatchFloat32: dst[i] = (src[i] OP val) ? 1 : 0, OP in simd.CompareOp order;
- simd.AndBytes: dst[i] &= src[i], bitwise;
- the Arrow validity rule of query.*FilterOp.MatchBitmap: row i is valid iff bit (i + offset) of the bitmap, LSB first,
  is set; nulls never match.
"""
import numpy as np

F = np.float32
EQ, NEQ, GT, GE, LT, LE = range(6)
OPS = (EQ, NEQ, GT, GE, LT, LE)

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
EDGE_N = 4099  # 256 full 16-element groups and one of 3: the last group is partial, the last mask store is not 16 bytes

# neighbours that differ only in the high word (5 / 2^32 + 5 / 2^62 + 5) or only in the low word (2^32 - 1 / 2^32 / 2^32 + 1),
# and both ends of the signed range: a 32-bit or an unsigned compare gets some (element, value, op) of these wrong
INT64_EDGES = (I64_MIN, I64_MIN + 1, -2 ** 32, -2 ** 32 - 1, -1, 0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1,
               2 ** 62 + 5, 5, I64_MAX - 1, I64_MAX)
INT64_VALUES = (I64_MIN, -1, 0, 5, 2 ** 32, 2 ** 32 + 5, 2 ** 62 + 5, I64_MAX)

FLT_MAX = float(np.finfo(F).max)
FLT_MIN = float(np.finfo(F).tiny)  # smallest normal
_NEG_NAN = np.array([0xFFC00000], np.uint32).view(F)[0]
FLOAT32_EDGES = (np.nan, _NEG_NAN, -np.inf, -FLT_MAX, -1.0, -FLT_MIN, -1e-40, -0.0, 0.0, 1.4e-45, 1e-40, FLT_MIN, 0.25, 1.0,
                 FLT_MAX, np.inf)
FLOAT32_VALUES = (-np.inf, -0.0, 0.0, 1e-40, 0.25, np.inf, np.nan)


def int64_edge_column(n=EDGE_N):
    return np.resize(np.array(INT64_EDGES, np.int64), n)


def float32_edge_column(n=EDGE_N):
    return np.resize(np.array(FLOAT32_EDGES, F), n)


# ---- restatements ---------------------------------------------------------------------------------------------------
def _compare(a, b, op):
    return (a == b, a != b, a > b, a >= b, a < b, a <= b)[op]


def match_int64(src, val, op):
    src = np.asarray(src, np.int64)
    return _compare(src, np.int64(val), op).astype(np.uint8)


def match_float32(src, val, op):
    """IEEE-754 binary32 comparison restated on the bit patterns, so that it does not depend on how the host's FPU is set up
    (flush-to-zero would hide the subnormals): NaN on either side makes `!=` true and every other operator false; otherwise
    the values order as sign-magnitude integers, with -0 and +0 the same key."""
    bits = np.ascontiguousarray(src, F).view(np.uint32).astype(np.int64)
    vbits = int(np.array([val], F).view(np.uint32)[0])

    def key(b):
        mag = b & 0x7FFFFFFF
        return np.where((b >> 31) != 0, -mag, mag)

    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    if (vbits & 0x7FFFFFFF) > 0x7F800000:
        nan = np.ones_like(nan)
    r = _compare(key(bits), key(np.int64(vbits)), op)
    return np.where(nan, op == NEQ, r).astype(np.uint8)


def and_bytes(dst, src):
    return np.bitwise_and(np.asarray(dst, np.uint8), np.asarray(src, np.uint8))


def validity(bitmap, offset, n):
    """valid[i] = bit (i + offset) of the Arrow bitmap, LSB first"""
    b = np.arange(n, dtype=np.int64) + offset
    return ((np.asarray(bitmap, np.uint8)[b >> 3] >> (b & 7).astype(np.uint8)) & 1).astype(np.uint8)


def validity_bitmap(valid, offset):
    """Arrow bitmap holding `valid` from bit `offset` on.  The `offset` bits in front are junk set to the opposite of
    valid[0] and the padding behind to the opposite of valid[-1], so reading one bit early or late shows."""
    valid = np.asarray(valid, bool)
    tail = -(offset + valid.size) % 8
    bits = np.concatenate([np.full(offset, not valid[0]), valid, np.full(tail, not valid[-1])])
    return np.packbits(bits, bitorder="little")


def predicate(col, val, op, valid=None):
    """expected row mask of filter_column: the match, ANDed with the validity"""
    col = np.asarray(col)
    m = match_int64(col, val, op) if col.dtype == np.int64 else match_float32(col, val, op)
    return m if valid is None else m & np.asarray(valid, np.uint8)


# ---- the second round of the grid-stride loops -----------------------------------------------------------------------
MATCH_ROUND = 4096 * 256 * 16  # elements match_kernel covers per round of its loop (the grid is capped at 4096 workgroups)
AND_ROUND = 4096 * 256
BIG_N = MATCH_ROUND + 48 + 5  # second round: three full 16-element groups and one of 5
# in the second round: start / inside / end of full groups, and the first and last element of the partial group; two more in
# the first round, so that a second round that re-reads the first one's elements shows as well
BIG_POSITIONS = (0, MATCH_ROUND - 1, MATCH_ROUND, MATCH_ROUND + 1, MATCH_ROUND + 15, MATCH_ROUND + 16, MATCH_ROUND + 47,
                 MATCH_ROUND + 48, MATCH_ROUND + 52)
BIG_INT64_CONST, BIG_INT64_VALUE = 5, 5
BIG_INT64_MARKS = (4, 6, 2 ** 32 + 5, I64_MIN, 6, 4, I64_MAX, -1, 2 ** 32 + 4)
BIG_FLOAT32_CONST, BIG_FLOAT32_VALUE = 0.25, 0.25
BIG_FLOAT32_MARKS = (0.5, -1.0, np.nan, 0.24999999, 0.5, -0.0, np.inf, -np.inf, 0.125)


def big_int64_column():
    a = np.full(BIG_N, BIG_INT64_CONST, np.int64)
    a[list(BIG_POSITIONS)] = np.array(BIG_INT64_MARKS, np.int64)
    return a


def big_float32_column():
    a = np.full(BIG_N, BIG_FLOAT32_CONST, F)
    a[list(BIG_POSITIONS)] = np.array(BIG_FLOAT32_MARKS, F)
    return a


# ---- masks ----------------------------------------------------------------------------------------------------------
MASK_BYTES = (0, 1, 2, 0x80, 0xFF)  # a row is visible iff its byte is not 0
CP_ROWS = 2048  # rows per workgroup of the compaction kernels (kernels_filter.hip: CP_THREADS * CP_PER)


def byte_mask(rng, n, visible_fraction):
    """mask bytes drawn from MASK_BYTES: 0 with probability 1 - visible_fraction, the four non-zero bytes equally else"""
    p = [1.0 - visible_fraction] + [visible_fraction / 4] * 4
    return rng.choice(np.array(MASK_BYTES, np.uint8), size=n, p=p)


def exact_count_mask(rng, n, n_visible, hidden=()):
    """0/1 mask with exactly n_visible visible rows, none of them in `hidden`"""
    m = np.zeros(n, np.uint8)
    m[rng.permutation(np.setdiff1d(np.arange(n), hidden))[:n_visible]] = 1
    return m


def takes_row_list(n_visible, n, max_pct=95):
    """rebuild_rowmap's rule (index.hip): searches walk the list of visible rows, not the per-row mask test"""
    return n_visible * 100 <= n * max_pct


def structured_masks(n, k, rng):
    """{name: 0/1 mask}: the visible rows where the compaction kernels and the list walkers have their edges"""
    def only(rows):
        m = np.zeros(n, np.uint8)
        m[np.asarray(rows, np.int64)] = 1
        return m

    last_block = (n - 1) // CP_ROWS * CP_ROWS
    out = {"row 0": only([0]), "row n-1": only([n - 1]), "last partial block": only(np.arange(last_block, n))}
    for c in (k - 1, k, k + 1):
        out[f"{c} rows spread"] = only(np.linspace(0, n - 1, c).round().astype(np.int64))
    starts = np.arange(0, n, CP_ROWS)
    spans = np.minimum(starts + CP_ROWS, n) - starts
    out["one row per block"] = only(starts + rng.integers(0, spans))
    m = np.ones(n, np.uint8)
    m[n // 3] = 0
    out["all but one"] = m
    return out
