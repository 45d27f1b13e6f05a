"""Inputs of the code handles' removal tests (tests/test_gpu_ivf_code_remove.py and tests/test_gpu_code_lifecycle.py on the GPU,
tests/test_ivf_code_remove_semantics.py on the CPU), for the IVF-PQ handle plain ("pq") and residual ("rpq") and the IVF-SQ8
handle ("sq8").  Everything is built from what the suite already has: each handle's oracle and its
parity_case / edge_case / skew_case, tests/remove_cases.py (ids, overlap sets, fractions) and tests/ivf_remove_cases.py (read-back
sets, the steps of the selection boundary).  Seeded, computed once per process, never written to.

A Kind is the one place that knows how a handle differs: how it is created, what its codes and its flat counterpart are, and which
oracle answers for it.  Every expected result is that oracle with mask = live & filter:
  pq   ivfpq_filter_cases.search_filtered         rpq  ivfpq_residual_oracle.search(..., visible=)
  sq8  ivfsq8_oracle.search(..., mask=)
The IVF-BQ handle has no removal entry points and no Kind here."""
import functools

import numpy as np

from tests import ivf_filter_cases as fc
from tests import ivf_remove_cases as vc
from tests import ivfpq_filter_cases as pfc
from tests import ivfpq_oracle as pqo
from tests import ivfpq_residual_oracle as rpo
from tests import ivfsq8_oracle as iso
from tests import remove_cases as rc

F = np.float32
FLT_MAX = np.finfo(F).max
NPROBES = vc.NPROBES            # (1, 4, 16)
KS = vc.KS                      # (1, 10, 100)
K_ALL = 2048
LDS_KEYS = fc.LDS_KEYS
ROUND_ROWS = 7                  # rows per round of a compaction in the diagnostic library
READBACK_NAMES = vc.READBACK_NAMES
live_mask, ids_for, overlap_sets, removed_rows, filter_mask, visible, counts = (rc.live_mask, rc.ids_for, rc.overlap_sets,
                                                                               rc.removed_rows, rc.filter_mask, vc.visible, vc.counts)


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


class Kind:
    """name, the scan's tile, the parity shapes, and the handle-specific calls.  `par`: what a handle is created from beside the
    centroids (codebooks / (min, max) / None)"""
    name = tile = None
    shapes = ()
    flat_equal = True  # with every list probed the handle equals the flat code handle over the same codes

    # inputs -> (X, Q, C, par)
    def parity_case(self, shape):
        raise NotImplementedError

    def edge_case(self):
        """-> (X, Q, C, owner, par)"""
        raise NotImplementedError

    def skew_case(self):
        raise NotImplementedError

    def small_case(self, dims, seed):
        """-> par for rows of `dims` dimensions that the caller brings (the lifecycle scripts)"""
        raise NotImplementedError

    # the oracle
    def assign(self, oracle, X, C, order=0):
        return pqo.assign(oracle, order, X, C)  # (ivf_oracle.assign at L2: the same for every kind)

    def encode(self, oracle, X, C, lists, par):
        raise NotImplementedError

    def search(self, oracle, Q, C, lists, codes, par, mask, k, nprobe, ids=None, order=0):
        """-> (labels, dist, rows scanned per query); mask: uint8 over the rows, live & filter"""
        raise NotImplementedError

    # the GPU
    def handle(self, C, par, order=0, lib=None):
        raise NotImplementedError

    def flat(self, codes, par, dims, lib=None):
        """the flat code handle holding `codes` -> an object with set_filter(mask), search(Q, k) and Close()"""
        raise NotImplementedError


class _Flat:
    def __init__(self, enc, search):
        self.enc, self.search = enc, search
        self.set_filter, self.Close = enc.set_filter, enc.Close


class PQ(Kind):
    name, tile, residual = "pq", pqo.TILE, False
    shapes = pqo.PARITY_SHAPES  # (dims, M): (16, 4) the byte form of the scan, (32, 16) the 16-byte form

    def parity_case(self, shape):
        return pqo.parity_case(*shape)

    def edge_case(self):
        return pqo.edge_case()

    def skew_case(self):
        return pqo.skew_case()

    def small_case(self, dims, seed):
        M = next(m for m in (8, 7, 4, 1) if dims % m == 0)
        return pqo.codebooks(dims, M, 900 + seed)

    def encode(self, oracle, X, C, lists, par):
        return pqo.encode(oracle, par, X)

    def search(self, oracle, Q, C, lists, codes, par, mask, k, nprobe, ids=None, order=0):
        return pfc.search_filtered(oracle, par, order, Q, C, lists, codes, mask, k, nprobe, ids=ids)

    def handle(self, C, par, order=0, lib=None):
        from longbow_amd import ivfpq
        return ivfpq.IVFPQ(pqo.blob(par), C, order, lib=lib, residual=self.residual)

    def flat(self, codes, par, dims, lib=None):
        from longbow_amd import pq
        enc = pq.PQEncoder(pqo.blob(par), lib=lib)
        enc.add_codes(codes)
        return _Flat(enc, enc.Search)


class RPQ(PQ):
    name, residual, flat_equal = "rpq", True, False  # (a residual handle's distances are per probed list: no flat counterpart)

    def encode(self, oracle, X, C, lists, par):
        return rpo.encode(oracle, par, X, C, lists)

    def search(self, oracle, Q, C, lists, codes, par, mask, k, nprobe, ids=None, order=0):
        return rpo.search(oracle, par, order, Q, C, lists, codes, k, nprobe, ids=ids, visible=mask)


class SQ8(Kind):
    name, tile = "sq8", iso.TILE
    shapes = (20, 768)  # dims: a padded stride (32 bytes for 20), and the workload's row

    def parity_case(self, shape):
        X, Q, C, mn, mx = iso.parity_case(shape)
        return X, Q, C, (mn, mx)

    def edge_case(self):
        X, Q, C, owner, mn, mx = iso.edge_case()
        return X, Q, C, owner, (mn, mx)

    def skew_case(self):
        X, Q, C, mn, mx = iso.skew_case()
        return X, Q, C, (mn, mx)

    def small_case(self, dims, seed):
        return np.full(dims, -8, F), np.full(dims, 8, F)  # (bounds fixed at creation; rows beyond them clamp, as SQ8 does)

    def encode(self, oracle, X, C, lists, par):
        return iso.encode(X, *par)

    def search(self, oracle, Q, C, lists, codes, par, mask, k, nprobe, ids=None, order=0):
        return iso.search(oracle, order, Q, C, lists, codes, par[0], par[1], k, nprobe, ids=ids, mask=mask)

    def handle(self, C, par, order=0, lib=None):
        from longbow_amd import ivfsq8
        return ivfsq8.IVFSQ8(par[0], par[1], C, order, lib=lib)

    def flat(self, codes, par, dims, lib=None):
        from longbow_amd import sq8
        enc = sq8.SQ8Encoder(dims, lib=lib)
        enc.set_bounds(*par)
        enc.add_codes(codes)
        return _Flat(enc, enc.search)


KINDS = {k.name: k for k in (PQ(), RPQ(), SQ8())}
# every (kind, parity shape) of the read-back test
SHAPES = [(name, shape) for name, k in KINDS.items() for shape in k.shapes]
SHAPE_IDS = [f"{name}-{'x'.join(map(str, shape)) if isinstance(shape, tuple) else shape}" for name, shape in SHAPES]
FIRST_SHAPE = {name: k.shapes[0] for name, k in KINDS.items()}


class Case:
    """one corpus of one kind with what the oracle derives from it: lists (order 0) and codes"""
    def __init__(self, oracle, kind, X, Q, C, par, lists=None):
        self.kind, self.k = kind, KINDS[kind]
        self.X, self.Q, self.C, self.par = X, Q, C, par
        self.n, self.dims, self.nlist = X.shape[0], X.shape[1], C.shape[0]
        self.lists = np.asarray(self.k.assign(oracle, X, C) if lists is None else lists, np.int64)
        self.codes = self.k.encode(oracle, X, C, self.lists, par)
        _ro(self.X, self.Q, self.C, self.lists, self.codes, *(par if isinstance(par, tuple) else (par,)))

    def search(self, oracle, Q, mask, k, nprobe, ids=None, rows=None):
        """the kind's oracle over rows `rows` of the case (None: all of them) under `mask` (over those rows)"""
        lists, codes = (self.lists, self.codes) if rows is None else (self.lists[rows], self.codes[rows])
        return self.k.search(oracle, Q, self.C, lists, codes, self.par, np.asarray(mask, np.uint8), k, nprobe, ids=ids)


@functools.lru_cache(maxsize=None)
def parity(oracle, kind, shape):
    """the kind's parity_case (n = 3,000, 16 lists, 33 queries) at `shape`"""
    X, Q, C, par = KINDS[kind].parity_case(shape)
    return Case(oracle, kind, X, Q, C, par)


@functools.lru_cache(maxsize=None)
def edge(oracle, kind):
    """the kind's edge_case: lists of (0, 1, TILE - 1, TILE, TILE + 1, several tiles and 77, 3, 5, 2, 0, 7) rows"""
    X, Q, C, owner, par = KINDS[kind].edge_case()
    return Case(oracle, kind, X, Q, C, par, lists=owner)


@functools.lru_cache(maxsize=None)
def skew(oracle, kind):
    """the kind's skew_case (50,000 rows, list 0 beyond what a selection holds in LDS) with ivf_remove_cases' eight queries"""
    X, Q5, C, par = KINDS[kind].skew_case()
    return Case(oracle, kind, X, vc.skew_queries(Q5), C, par)


@functools.lru_cache(maxsize=None)
def grown(oracle, kind):
    """the kind's first parity case with 2,000 more standard-normal rows behind it: 5,000 rows, for the adds after a removal"""
    c = parity(oracle, kind, FIRST_SHAPE[kind])
    more = np.random.default_rng(7).standard_normal((2000, c.dims)).astype(F)
    return Case(oracle, kind, np.concatenate([c.X, more]), c.Q, c.C, c.par)


def readback_sets(lists):
    return vc.readback_sets(lists)


def queries(case, removed):
    """the case's queries with query 0 replaced by a removed row's own vector"""
    return rc.queries(case.X, case.Q, removed)


def edge_keeps(kind):
    """name -> live rows each list of edge(kind) is left.  A: emptied lists, 1, TILE - 1, TILE and TILE + 1 (the last thinned from
    the long list); B: one list of several tiles plus one row, longer than one step of the scan's stride loop at the case's
    queries (8 workgroups a query on IVF-PQ, 16 along a list on IVF-SQ8), beside 0, 1, TILE and TILE + 1"""
    T = KINDS[kind].tile
    long_b = (8 if kind in ("pq", "rpq") else 16) * T + 1
    return {"A": (0, 0, T - 1, T - 1, T, T + 1, 3, 1, 0, 0, 7), "B": (0, 1, 0, T, T + 1, long_b, 2, 5, 1, 0, 0)}


def edge_removed(owner, keep, rng=None):
    return np.flatnonzero(fc.keep_per_list(owner, keep, rng) == 0).astype(np.int64)


skew_steps = vc.skew_steps
SKEW_KEEP = vc.SKEW_KEEP


def back(labels, keep):
    """labels of a handle of the survivors alone, without ids -> the old positions (old_rows)"""
    keep = np.asarray(keep, np.int64)
    return np.where(labels >= 0, np.append(keep, -1)[np.clip(labels, 0, None)], -1)


def same_handles(h, fresh, Q, ctx, ks=KS, nprobes=NPROBES):
    """two code handles on a GPU answer alike and hold the same codes: h (compacted) is what an add of the survivors (fresh) would
    have made"""
    vc.same_handles(h, fresh, Q, ctx, ks=ks, nprobes=nprobes)
    assert np.array_equal(h.codes(), fresh.codes()), f"{ctx}: the codes"
