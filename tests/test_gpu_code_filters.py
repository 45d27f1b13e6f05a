"""Row filters on the BQ and SQ8 indexes (lb_gpu_bq_* / lb_gpu_sq8_* set_filter, filter_int64 / _float32, nvisible) on the GPU.
The expected result everywhere is the numpy oracle on the visible subset (tests/code_filter_cases.py: subset_search, pinned on
the CPU by tests/test_code_filter_semantics.py); labels and distances are compared for equality."""
import functools
import os
import re

import numpy as np
import pytest

from tests import code_filter_cases as cf
from tests import row_view_cases as rv
from tests.gpu_util import gpu_or_skip, new_index

pytestmark = pytest.mark.gpu
F = np.float32
FLT_MAX = cf.FLT_MAX
CASES = [("bq", d) for d in cf.BQ_DIMS] + [("sq8", d) for d in cf.SQ8_DIMS]
KINDS = [("bq", 64), ("sq8", 16)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enc(kind, dims):
    gpu_or_skip()
    from longbow_amd import bq, sq8
    return bq.BQEncoder(dims) if kind == "bq" else sq8.SQ8Encoder(dims)


@functools.lru_cache(maxsize=None)
def _corpus(kind, dims):
    """(codes [N], query codes [17]) of one (index, dims): computed once, shared by the mask cases, never written to"""
    rng = np.random.default_rng(dims * 13 + len(kind))
    codes = cf.codes_of(kind, rng, cf.N, dims)
    q = cf.codes_of(kind, rng, max(cf.NQS), dims)
    q[0] = codes[cf.N // 2]
    codes.setflags(write=False)
    q.setflags(write=False)
    return codes, q


def _check(enc, kind, q, codes, mask, k, ctx):
    lab, dist = enc.search_codes(q, k)
    wlab, wdist = cf.subset_search(kind, q, codes, mask, k)
    assert np.array_equal(lab, wlab), f"labels differ {ctx}: {np.argwhere(lab != wlab)[:5]}"
    assert np.array_equal(dist, wdist), f"distances differ {ctx}"
    return lab, dist


# ---- every mask, every dims, nq in {1, 5, 17}, k in {1, 10, 100} ---------------------------------------------------------------
@pytest.mark.parametrize("k", cf.KS)
@pytest.mark.parametrize("kind,dims", CASES)
def test_masked_search_equals_the_oracle_on_the_visible_rows(kind, dims, k):
    codes, q = _corpus(kind, dims)
    enc = _enc(kind, dims)
    enc.add_codes(codes)
    rng = np.random.default_rng(dims + k)
    for name, mask in cf.masks(cf.N, k, rng).items():
        enc.set_filter(mask)
        nvis = int(np.count_nonzero(mask))
        assert enc.nvisible() == nvis and enc.ntotal == cf.N, name
        wlab, wdist = cf.subset_search(kind, q, codes, mask, k)  # (17 queries; a smaller batch is its first rows)
        for nq in cf.NQS:
            lab, dist = enc.search_codes(q[:nq], k)
            assert np.array_equal(lab, wlab[:nq]), f"labels differ: {name}, {kind} {dims}, nq {nq}, k {k}: {np.argwhere(lab != wlab[:nq])[:5]}"
            assert np.array_equal(dist, wdist[:nq]), f"distances differ: {name}, {kind} {dims}, nq {nq}, k {k}"
            if name.endswith("rows spread") or name == "all-zero":  # the padding: the visible rows first, then -1 / FLT_MAX
                have = min(k, nvis)
                assert (lab[:, :have] >= 0).all() and (lab[:, have:] == -1).all() and (dist[:, have:] == FLT_MAX).all(), (name, nq)
    enc.Close()


# ---- ties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims", KINDS + [("bq", 768), ("sq8", 100)])
def test_identical_codes_under_a_mask_return_the_lowest_visible_rows(kind, dims):
    rng = np.random.default_rng(dims)
    codes = np.repeat(cf.codes_of(kind, rng, 1, dims), cf.N, axis=0)
    q = np.concatenate([codes[:1], cf.codes_of(kind, rng, 4, dims)])
    mask = rv.byte_mask(rng, cf.N, 0.5)
    vis = np.flatnonzero(mask)
    enc = _enc(kind, dims)
    enc.add_codes(codes)
    enc.set_filter(mask)
    for k in (1, 10, 300):  # 300: more than one tile of the list
        lab, dist = _check(enc, kind, q, codes, mask, k, f"{kind} {dims} k {k}")
        assert (lab == vis[:k]).all() and (dist[0] == 0).all()
    enc.Close()


@pytest.mark.parametrize("kind,dims", KINDS + [("bq", 1100), ("sq8", 768)])
def test_duplicates_across_a_tile_and_workgroup_boundary_of_the_list(kind, dims):
    """A block of rows equal to the query at list positions 250 .. 261: it straddles positions 255 / 256, where one 256-row tile
    and (5003 rows: one tile per workgroup) one workgroup of the list ends; in the corpus the block lies at rows 376 .. 392,
    inside tile 1.  The hidden rows between them are duplicates too and must not come back."""
    codes, q17 = _corpus(kind, dims)
    codes = codes.copy()
    mask = (np.arange(cf.N) % 3 != 0).astype(np.uint8)
    vis = np.flatnonzero(mask)
    block = vis[250:262]
    assert block[0] // 256 == block[-1] // 256 == 1 and block[5] == vis[255] and block[6] == vis[256]
    codes[block[0]:block[-1] + 1] = q17[1]  # the visible ones and the hidden ones between them
    assert (mask[block[0]:block[-1] + 1] == 0).sum() >= 5
    q = q17[1:4]
    enc = _enc(kind, dims)
    enc.add_codes(codes)
    enc.set_filter(mask)
    for k in (6, 8, 12, 20):
        lab, dist = _check(enc, kind, q, codes, mask, k, f"{kind} {dims} k {k}")
        m = min(k, 12)
        assert np.array_equal(lab[0, :m], block[:m]) and (dist[0, :m] == 0).all()
    enc.Close()


# ---- more than one tile per workgroup under a list -------------------------------------------------------------------------------
def _cap(name):
    with open(os.path.join(ROOT, "longbow_amd", "csrc", "lb_device.h")) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


@pytest.mark.parametrize("kind,dims,cap_name,rows", [("bq", 64, "BQ_MAX_BLOCKS", 700_001), ("sq8", 16, "SQ8_MAX_BLOCKS", 300_001)])
def test_a_list_longer_than_one_tile_per_workgroup(kind, dims, cap_name, rows):
    cap = _cap(cap_name)
    n = max(rows, int(cap * 256 / 0.9 * 1.03) + 1)  # about 90 % visible is still more than cap tiles
    rng = np.random.default_rng(cap)
    codes = cf.codes_of(kind, rng, n, dims)
    q = cf.codes_of(kind, rng, 3, dims)
    mask = rv.byte_mask(rng, n, 0.9)
    enc = _enc(kind, dims)
    enc.add_codes(codes)
    enc.set_filter(mask)
    tiles = -(-enc.nvisible() // 256)
    assert enc.nvisible() == np.count_nonzero(mask) and -(-tiles // cap) >= 2, "the list must take two tiles per workgroup"
    _check(enc, kind, q, codes, mask, 10, f"{kind} n {n}")
    enc.Close()


# ---- life cycle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims", KINDS + [("bq", 768), ("sq8", 100)])
def test_filter_life_cycle(kind, dims):
    from longbow_amd import _lib
    codes, q17 = _corpus(kind, dims)
    q, k = q17[:5], 10
    rng = np.random.default_rng(3)
    enc = _enc(kind, dims)
    enc.add_codes(codes)
    assert enc.nvisible() == cf.N
    first = enc.search_codes(q, k)
    mask = rv.byte_mask(rng, cf.N, 0.3)
    enc.set_filter(mask)
    _check(enc, kind, q, codes, mask, k, "set")
    # what addresses rows directly ignores the filter
    hidden = np.flatnonzero(mask == 0)[:7]
    assert np.array_equal(enc.get_codes(int(hidden[0]), 1), codes[hidden[:1]])
    if kind == "bq":
        assert np.array_equal(enc.HammingDistanceBatch(q[1]), cf.bo.hamming(q[1], codes))
        assert np.array_equal(enc.rerank(q[1], hidden, want_score=False), cf.bo.hamming(q[1], codes[hidden]).astype(F))
    else:
        assert np.array_equal(enc.distance_batch(q[1]), cf.so.dist_s(q[1], codes))
        assert np.array_equal(enc.rerank(q[1], hidden, want_euclid=False), cf.so.dist_s(q[1], codes[hidden]))
    # a mask of the wrong length is refused and the old filter still holds
    for bad in (mask[:-1], np.concatenate([mask, mask[:1]])):
        with pytest.raises(_lib.LongbowGPUError) as e:
            enc.set_filter(bad)
        assert e.value.code == 1 and "rows" in str(e.value)
    with pytest.raises(_lib.LongbowGPUError):
        enc.filter_column(np.zeros(cf.N - 1, np.int64), 0, rv.EQ)
    assert enc.nvisible() == np.count_nonzero(mask)
    _check(enc, kind, q, codes, mask, k, "after the refusals")
    # rows added under a filter are visible, across a growth of the buffers too (5003 -> 9003 rows)
    more = cf.codes_of(kind, rng, 4000, dims)
    more[:3] = q[:3]
    enc.add_codes(more)
    both, mask2 = np.concatenate([codes, more]), np.concatenate([mask, np.ones(4000, np.uint8)])
    assert enc.ntotal == cf.N + 4000 and enc.nvisible() == np.count_nonzero(mask) + 4000
    lab, _ = _check(enc, kind, q, both, mask2, k, "after add_codes")
    assert cf.N in lab[0] and cf.N + 1 in lab[1]  # the added copies of the queries are found
    # clearing returns the unfiltered result of the grown index; the first result comes back on a handle cleared before the add
    enc.set_filter(None)
    assert enc.nvisible() == enc.ntotal
    _check(enc, kind, q, both, np.ones(both.shape[0], np.uint8), k, "cleared")
    enc.Close()
    enc = _enc(kind, dims)
    enc.add_codes(codes)
    enc.set_filter(mask)
    enc.set_filter(None)
    again = enc.search_codes(q, k)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    # rows added to a cleared handle are plain rows, and a filter set on an empty handle covers what is added later
    enc.Close()
    enc = _enc(kind, dims)
    enc.set_filter(np.zeros(0, np.uint8))
    assert enc.nvisible() == 0
    enc.add_codes(codes[:300])
    assert enc.nvisible() == 300
    _check(enc, kind, q, codes[:300], np.ones(300, np.uint8), k, "filter set on an empty handle")
    enc.Close()


def test_vectors_added_under_a_filter_are_visible():
    from longbow_amd import bq, sq8
    gpu_or_skip()
    rng = np.random.default_rng(9)
    dims, n = 100, 700
    X = (rng.random((n, dims), dtype=F) - F(0.5)).astype(F)
    Q = (rng.random((3, dims), dtype=F) - F(0.5)).astype(F)
    mask = rv.byte_mask(rng, n, 0.5)
    for kind in ("bq", "sq8"):
        enc = bq.BQEncoder(dims) if kind == "bq" else sq8.train(X)
        enc.add_vectors(X)
        enc.set_filter(mask)
        enc.add_vectors(X[:50])
        assert enc.nvisible() == np.count_nonzero(mask) + 50
        codes = enc.get_codes()
        lab, dist = enc.search(Q, 20)
        wlab, wdist = cf.subset_search(kind, enc.Encode(Q), codes, np.concatenate([mask, np.ones(50, np.uint8)]), 20)
        assert np.array_equal(lab, wlab) and np.array_equal(dist, wdist), kind
        enc.Close()


# ---- predicates evaluated on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dims", KINDS)
def test_filter_column_equals_the_restated_predicate(kind, dims):
    n, k = rv.EDGE_N, 10
    rng = np.random.default_rng(17)
    codes = cf.codes_of(kind, rng, n, dims)
    q = cf.codes_of(kind, rng, 5, dims)
    icol, fcol = rv.int64_edge_column(n), rv.float32_edge_column(n)
    ivalid, fvalid = rng.random(n) < 0.8, rng.random(n) < 0.8
    enc = _enc(kind, dims)
    enc.add_codes(codes)
    # combine on a handle without a filter replaces the mask
    enc.filter_column(icol, 2 ** 32, rv.GE, valid=rv.validity_bitmap(ivalid, 3), validity_offset=3, combine=True)
    m1 = rv.predicate(icol, 2 ** 32, rv.GE, ivalid)
    assert 0 < m1.sum() < n and enc.nvisible() == m1.sum()
    _check(enc, kind, q, codes, m1, k, "int64 GE, combine on no filter")
    # combine 0 replaces, combine 1 ANDs into it
    enc.filter_column(fcol, 0.25, rv.LE, valid=rv.validity_bitmap(fvalid, 5), validity_offset=5, combine=False)
    m2 = rv.predicate(fcol, 0.25, rv.LE, fvalid)
    assert 0 < m2.sum() < n and enc.nvisible() == m2.sum()
    _check(enc, kind, q, codes, m2, k, "float32 LE, replace")
    enc.filter_column(icol, 5, "!=", valid=rv.validity_bitmap(ivalid, 3), validity_offset=3, combine=True)
    m3 = rv.and_bytes(m2, rv.predicate(icol, 5, rv.NEQ, ivalid))
    assert 0 < m3.sum() < m2.sum() and enc.nvisible() == m3.sum()
    _check(enc, kind, q, codes, m3, k, "int64 NEQ, combined")
    with pytest.raises(TypeError):
        enc.filter_column(icol.astype(np.int32), 5, rv.EQ)
    enc.Close()


# ---- the two-stage search --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bq", "sq8"])
def test_search_rerank_under_a_mask_returns_visible_rows_only(kind, oracle):
    from longbow_amd import bq, sq8
    gpu_or_skip()
    n, dims, nq, k, over = 20000, 128, 4, 10, 10
    rng = np.random.default_rng(78)
    X = (rng.random((n, dims), dtype=F) - F(0.5)).astype(F)
    Q = (X[rng.integers(0, n, nq)] + F(0.05) * (rng.random((nq, dims), dtype=F) - F(0.5))).astype(F)
    mask = rv.byte_mask(rng, n, 0.10)
    enc = bq.BQEncoder(dims) if kind == "bq" else sq8.train(X)
    enc.add_vectors(X)
    enc.set_filter(mask)
    idx = new_index(dims, 0)
    idx.Add(None, X)
    lab, dist = enc.search_rerank(idx, Q, k, over)
    assert (lab >= 0).all() and (mask[lab] != 0).all()
    short, _ = cf.subset_search(kind, enc.Encode(Q), enc.get_codes(), mask, k * over)
    for i in range(nq):
        d = oracle.batch_flat(0, Q[i], X[short[i]], 1)
        keep = np.lexsort((short[i], d))[:k]
        assert np.array_equal(lab[i], short[i][keep]) and np.array_equal(dist[i], d[keep])
    idx.Close()
    enc.Close()
