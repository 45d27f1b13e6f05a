"""Inputs of the removal tests (tests/test_gpu_remove.py on the GPU, tests/test_remove_semantics.py on the CPU): corpora, removal
sets, ids, filters and the map from old labels to survivors.  Seeded, computed once per process, never written to."""
import functools

import numpy as np

F = np.float32
L2, COS, DOT = 0, 1, 2
SMALL = (2049, 8)     # read-back: k = 2048 returns every live row
MAIN = (20000, 32)    # the route classes of the views
ODD = (20000, 100)    # a dimension that is no multiple of 32
NQS = (1, 8, 64, 385)
KS = (1, 10, 100)
# removed fraction -> the route class it lands in (index.hip: rebuild_rowmap keeps the per-row mask test above 95 % visible;
# index_search.hip samples a threshold and offers the fp16 image from 16,384 rows of the view)
FRACTIONS = {"2pct": 0.02, "18pct": 0.18, "60pct": 0.60}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def corpus(shape, seed=700):
    """(X [n, d], Q [385, d]) uniform [0, 1) f32"""
    rng = np.random.default_rng(seed + shape[0] + shape[1])
    return _ro(rng.random(shape, dtype=F), rng.random((NQS[-1], shape[1]), dtype=F))


@functools.lru_cache(maxsize=None)
def removed_rows(n, name):
    """the ascending rows a fraction removes"""
    cnt = int(round(n * FRACTIONS[name]))
    rows = np.sort(np.random.default_rng(int(FRACTIONS[name] * 1000) + n).choice(n, cnt, replace=False)).astype(np.int64)
    return _ro(rows)


def live_mask(n, removed):
    live = np.ones(n, np.uint8)
    live[np.asarray(removed, np.int64)] = 0
    return live


def queries(X, Q, removed):
    """Q with query 0 replaced by a removed row's own vector: its true nearest neighbour is a row that must not appear"""
    Q = Q.copy()
    if len(removed):
        Q[0] = X[removed[len(removed) // 2]]
    return _ro(Q)


def readback_sets(n):
    """name -> removed rows of the read-back test"""
    every_other = np.arange(0, n, 2)
    return {"none": np.empty(0, np.int64), "first": np.array([0]), "last": np.array([n - 1]), "every other": every_other,
            "all but one": np.delete(np.arange(n), n // 3), "all": np.arange(n)}


def overlap_sets(n):
    """name -> removed rows of the compaction's overlap cases: every row shifts by one, none overlaps, a block, alternating"""
    return {"row 0": np.array([0]), "first half": np.arange(n // 2), "middle block": np.arange(n // 3, n // 3 + n // 5),
            "every other": np.arange(0, n, 2)}


def ids_for(n):
    """distinct int64 ids with negatives and values beyond 2^32, none of them -1"""
    ids = np.arange(n, dtype=np.int64) * 1_000_003_001 - 5_000_000_000
    assert ids[0] < 0 and ids[-1] > 2 ** 32 and not (ids == -1).any() and np.unique(ids).size == n
    return ids


def filter_mask(n, seed=5, fraction=0.7):
    return (np.random.default_rng(seed).random(n) < fraction).astype(np.uint8)


def gpu_cases():
    """every (tag, shape, removed rows, with ids) whose searches the GPU file compares with the oracle"""
    out = []
    for name, rows in readback_sets(SMALL[0]).items():
        out.append((f"readback {name}", SMALL, rows, False))
    for name in FRACTIONS:
        out.append((f"views {name}", MAIN, removed_rows(MAIN[0], name), False))
        out.append((f"views {name} ids", MAIN, removed_rows(MAIN[0], name), True))
    out.append(("views 18pct dim 100", ODD, removed_rows(ODD[0], "18pct"), False))
    for shape in (SMALL, MAIN):
        for name, rows in overlap_sets(shape[0]).items():
            out.append((f"overlap {name} {shape[0]}", shape, rows, False))
    return out
