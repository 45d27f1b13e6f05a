"""Inputs and the two statements of a filtered k-NN over codes, shared by tests/test_code_filter_semantics.py (CPU: the two
statements are shown to agree) and tests/test_gpu_code_filters.py (GPU: the BQ and SQ8 indexes are compared with the first).

The expected result is the existing numpy oracle on the visible subset: vis = flatnonzero(mask), the oracle's search over
codes[vis], labels mapped back through vis with -1 kept (`subset_search`).  The independent statement is the full distance
matrix with the hidden rows at +inf and a stable argsort per query, i.e. ascending by (distance, row) (`masked_topk`)."""
import numpy as np

from tests import bq_oracle as bo
from tests import row_view_cases as rv
from tests import sq8_oracle as so

F = np.float32
FLT_MAX = np.finfo(F).max
N = 5003                 # the last 256-row tile is partial and the rows take several workgroups
NQS = (1, 5, 17)         # a single query, a part-filled tile of 8, two query tiles
KS = (1, 10, 100)
BQ_DIMS = (64, 768, 1100)   # W = 1 (chunks of 4 with zero words), W = 12 (one chunk), W = 18 (three chunks of 8, pad bits)
SQ8_DIMS = (16, 100, 768)   # one piece, stride 112 with pad bytes, 48 pieces


def masks(n, k, rng):
    """{name: mask}: tests/row_view_cases.py's structured masks, byte masks at 10 % and 50 % (bytes 1, 2, 0x80, 0xFF), none, all"""
    out = dict(rv.structured_masks(n, k, rng))
    out["10 % byte mask"] = rv.byte_mask(rng, n, 0.10)
    out["50 % byte mask"] = rv.byte_mask(rng, n, 0.50)
    out["all-zero"] = np.zeros(n, np.uint8)
    out["all-one"] = np.ones(n, np.uint8)
    return out


def bq_codes(rng, n, dims):
    """uniform random bits, pad bits zero"""
    W = bo.words(dims)
    c = rng.integers(0, 1 << 64, (n, W), dtype=np.uint64)
    if dims % 64:
        c[:, -1] &= np.uint64((1 << (dims % 64)) - 1)
    return c


def sq8_codes(rng, n, dims):
    """bytes over the whole range at 768 dimensions, over four values below (so that equal distances are common)"""
    return rng.integers(0, 256 if dims >= 768 else 4, (n, dims), dtype=np.uint8)


def oracle_of(kind):
    return bo if kind == "bq" else so


def codes_of(kind, rng, n, dims):
    return bq_codes(rng, n, dims) if kind == "bq" else sq8_codes(rng, n, dims)


def dist_matrix(kind, qcodes, codes):
    """every query against every row -> int64 [nq, n]"""
    if kind == "bq":
        return np.stack([bo.hamming(q, codes).astype(np.int64) for q in np.asarray(qcodes).reshape(-1, codes.shape[1])])
    return so.dist_matrix(qcodes, codes)


def subset_search(kind, qcodes, codes, mask, k):
    """the oracle's k-NN over the visible rows alone, labels mapped back to corpus rows -> (labels [nq, k], dist [nq, k])"""
    vis = np.flatnonzero(mask)
    lab, dist = oracle_of(kind).search(qcodes, codes[vis], k)
    return np.where(lab >= 0, vis[np.clip(lab, 0, max(vis.size - 1, 0))] if vis.size else -1, -1).astype(np.int64), dist


def masked_topk(D, mask, k):
    """hidden rows at +inf, then per query the first k of a stable argsort: ascending by (distance, row)"""
    D = np.asarray(D).astype(np.float64)  # (the integers are below 2^31: exact)
    D[:, np.asarray(mask) == 0] = np.inf
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    picked = np.take_along_axis(D, order, axis=1)
    labels = np.full((D.shape[0], k), -1, np.int64)
    dist = np.full((D.shape[0], k), FLT_MAX, F)
    ok = np.isfinite(picked)
    labels[:, :order.shape[1]] = np.where(ok, order, -1)
    dist[:, :order.shape[1]] = np.where(ok, picked, FLT_MAX).astype(F)
    return labels, dist
