"""A model of the handles that can forget rows (the flat index, lb_gpu_index_*, and the IVF-Flat handle, lb_gpu_ivf_*), written from
include/longbow_gpu.h alone, and seeded scripts of add / filter / remove / compact calls to drive a handle and the model side by
side (tests/test_gpu_lifecycle.py on the GPU; tests/test_lifecycle_model_semantics.py pins the model and the scripts on the CPU).
Pure numpy: no GPU, no torch.  What needs the C oracle (the lists of rows, the expected searches) takes it as an argument, as the
other *_cases.py files do.

Model        the physical rows as the handle stores them, their widened float32 copy, ids or None, `live`, the caller's `mask` or
             None, and one method per handle operation that returns what the handle must return.
script       a deterministic list of about 40 operations from a weighted grammar: single operations with random arguments and
             short fixed sequences ("blocks") that reach the states no fixed test reaches.  The generator redraws until coverage()
             and missing() find that it lacks nothing of what is asked of its seed.
coverage     replays a script on a fresh Model and reports which operations, states and edge conditions occurred."""
import functools

import numpy as np

from tests import row_view_cases as rv

F = np.float32
KINDS = ("f32", "f16", "i8")
DTYPES = {"f32": np.float32, "f16": np.float16, "i8": np.int8}
SEEDS = (0, 1, 2)
# every (kind, with_ids, seed) the GPU test runs; the CPU test asserts the model and the coverage for exactly these
PARAMS = [(kind, with_ids, seed) for kind in KINDS for with_ids in (False, True) for seed in SEEDS]
DIAG = {(kind, True, 0) for kind in KINDS}  # the scripts that run in the diagnostic library with compaction rounds of 7 rows
# seed -> (metric, order): every metric the kind supports occurs, and both orders for f32 (int8: the order is the coarse index's)
METRIC_ORDER = {"f32": ((0, 0), (1, 1), (2, 0)), "f16": ((0, 1), (1, 0), (2, 1)), "i8": ((0, 0), (2, 1), (0, 1))}
NLIST = 8
NQ = 9
KS = (1, 10)
K_PAD = 64            # also searched on the steps marked k64
MAX_ROWS = 8000       # the physical rows stay below this
MAX_ADD = 2500
ROUND_ROWS = 7
UNKNOWN_ID = 123456789012345
MUTATING = ("add", "reserve", "set_filter", "filter_column", "remove", "remove_rows", "remove_device", "compact")
STATES = ("remove a row added after a compaction, by id, beside ids that left",
          "compact under a filter, clear it, remove, compact",
          "compact to empty under a filter, then add",
          "remove, grow under a filter, filter_column combine, remove",
          "remove by the same labels after a renumbering compaction",
          "a compaction with nothing removed, live bytes allocated",
          "an add into a live word that holds removed rows")
IDS_ONLY, NO_IDS_ONLY = STATES[0], STATES[4]


def shape_of(kind, with_ids, seed):
    """-> (dim, metric, order): 24 dimensions (rows of 96, 48 and 24 bytes: the gather's 16- and 8-byte pieces), and 7 in one f32
    script (28 bytes: the 4-byte piece)"""
    metric, order = METRIC_ORDER[kind][seed % 3]
    return (7 if (kind, with_ids, seed) == ("f32", False, 2) else 24), metric, order


# capacity rules of the two handles (index.hip: grow; lb_handle.h: grow_capacity): the model keeps them to know when an add grows
def flat_capacity(cap, need):
    return cap if need <= cap else max(need, cap * 2, 1024)


def ivf_capacity(cap, need):
    return cap if need <= cap else max(need, cap * 2, 4096)


def widen(kind, rows):
    return np.ascontiguousarray(rows, DTYPES[kind]).astype(F)


class Model:
    def __init__(self, kind, dim, with_ids, assign=None):
        """assign: rows widened to f32 -> the list of each (the oracle's); None: the model keeps no lists"""
        self.kind, self.dim, self.with_ids, self.assign = kind, dim, with_ids, assign
        self.rows = np.empty((0, dim), DTYPES[kind])
        self.wide = np.empty((0, dim), F)
        self.ids = np.empty(0, np.int64) if with_ids else None
        self.live = np.empty(0, np.uint8)
        self.mask = None
        self.lists = None if assign is None else np.empty(0, np.int64)
        self.flat_cap = self.ivf_cap = 0
        self.grew = (False, False)  # did the last add or reserve grow the flat index / the IVF handle

    # ---- state ----
    @property
    def ntotal(self):
        return self.live.size

    def visible(self):
        return (self.live != 0) if self.mask is None else (self.live != 0) & (self.mask != 0)

    def counts(self):
        """(ntotal, nlive, ndeleted, nvisible)"""
        nlive = int(np.count_nonzero(self.live))
        return self.ntotal, nlive, self.ntotal - nlive, int(np.count_nonzero(self.visible()))

    def labels(self):
        """what a search returns for each physical row"""
        return np.arange(self.ntotal, dtype=np.int64) if self.ids is None else self.ids

    def _grow(self, need):
        f, v = flat_capacity(self.flat_cap, need), ivf_capacity(self.ivf_cap, need)
        self.grew = (f != self.flat_cap, v != self.ivf_cap)
        self.flat_cap, self.ivf_cap = f, v

    # ---- the operations ----
    def add(self, rows, ids=None):
        rows = np.ascontiguousarray(rows, DTYPES[self.kind]).reshape(-1, self.dim)
        assert (ids is not None) == self.with_ids, "ids on every add or on none"
        n = rows.shape[0]
        self._grow(self.ntotal + n)
        w = widen(self.kind, rows)
        self.rows, self.wide = np.concatenate([self.rows, rows]), np.concatenate([self.wide, w])
        if self.with_ids:
            self.ids = np.concatenate([self.ids, np.asarray(ids, np.int64).reshape(-1)])
        self.live = np.concatenate([self.live, np.ones(n, np.uint8)])       # rows added later are live
        if self.mask is not None:
            self.mask = np.concatenate([self.mask, np.ones(n, np.uint8)])   # and visible
        if self.lists is not None:
            self.lists = np.concatenate([self.lists, np.asarray(self.assign(w), np.int64)])

    def reserve(self, n):
        self._grow(n)

    def set_filter(self, mask):
        if mask is None:
            self.mask = None
            return
        mask = np.array(mask, np.uint8).reshape(-1)
        assert mask.size == self.ntotal, "a filter takes ntotal values, removed rows included"
        self.mask = mask

    def filter_column(self, column, op, value, combine=False):
        column = np.asarray(column)
        assert column.size == self.ntotal and column.dtype in (np.int64, np.float32)
        pred = rv.predicate(column, value, op)
        self.mask = rv.and_bytes(self.mask, pred) if combine and self.mask is not None else pred

    def _take(self, rows):
        """rows: a boolean vector over the physical rows -> the live ones among them go"""
        go = rows & (self.live != 0)
        self.live[go] = 0
        return int(np.count_nonzero(go))

    def remove_rows(self, pos):
        pos = np.asarray(pos, np.int64).reshape(-1)
        pos = pos[(pos >= 0) & (pos < self.ntotal)]  # (-1 and positions outside [0, ntotal) are ignored)
        hit = np.zeros(self.ntotal, bool)
        hit[pos] = True                              # (a position given twice counts once)
        return self._take(hit)

    def remove(self, labels):
        labels = np.asarray(labels, np.int64).reshape(-1)
        if self.ids is None:
            return self.remove_rows(labels)
        return self._take(np.isin(self.ids, labels[labels != -1]))  # every live row under an id goes; unknown ids name no row

    remove_device = remove

    def compact(self):
        keep = np.flatnonzero(self.live)
        self.rows, self.wide = self.rows[keep], self.wide[keep]
        if self.ids is not None:
            self.ids = self.ids[keep]
        if self.mask is not None:
            self.mask = self.mask[keep]
        if self.lists is not None:
            self.lists = self.lists[keep]
        self.live = np.ones(keep.size, np.uint8)
        return keep.astype(np.int64)

    def survivors(self):
        """what a fresh handle of the live rows is built from -> (keep, rows, widened rows, ids, restricted mask, lists)"""
        keep = np.flatnonzero(self.live)
        pick = lambda a: None if a is None else a[keep]
        return keep, self.rows[keep], self.wide[keep], pick(self.ids), pick(self.mask), pick(self.lists)


# ---- expected searches: the oracle over all physical rows with visible = live & mask --------------------------------------
def expect_flat(oracle, m, metric, order, Q, k):
    from tests import i8_oracle
    vis = m.visible()
    if m.kind == "i8":
        return i8_oracle.search(metric, Q, m.rows, k, ids=m.ids, visible=np.flatnonzero(vis))
    return oracle.search_batch(metric, np.asarray(Q, F), m.wide, k, order=order, mask=vis.astype(np.uint8), ids=m.ids, nthreads=8)


def expect_ivf(oracle, m, metric, order, Q, C, k, nprobe):
    """-> (labels, dist, rows scanned per query)"""
    from tests import ivf_remove_cases as vc
    ids = m.ids if m.ntotal else None  # (an empty handle: all padding, and no id to look up)
    if m.kind == "i8":
        return vc.search_live_i8(oracle, metric, order, Q, m.rows, C, m.lists, m.live, k, nprobe, ids=ids, mask=m.mask)
    return vc.search_live(oracle, metric, order, np.asarray(Q, F), m.wide, C, m.lists, m.live, k, nprobe, ids=ids, mask=m.mask)


def assigner(oracle, metric, order, C):
    from tests import ivf_oracle as io
    return lambda wide: io.assign(oracle, metric, order, wide, C)


def forbidden_labels(m):
    """labels no search may return: those of removed or hidden rows that no visible row carries too"""
    lab, vis = m.labels(), m.visible()
    return np.setdiff1d(lab[~vis], lab[vis])


# ---- scripts --------------------------------------------------------------------------------------------------------------
class Op:
    """one step: the call, its arguments, and the search check behind it (queries Q in the handle's query type, whether k = 64 is
    searched too, whether the device-pointer forms are used, and on every fifth step a shortlist for Refine and Rerank)"""
    def __init__(self, name, **args):
        self.name, self.args = name, args
        self.Q = self.short = None
        self.k64 = self.device = False

    def __str__(self):
        def show(v):
            if isinstance(v, np.ndarray):
                if v.size <= 8:
                    return f"{v.dtype}{v.tolist()}"
                return f"{v.dtype}[{'x'.join(map(str, v.shape))}] first {v.reshape(-1)[:4].tolist()} sum {int(np.asarray(v, np.float64).sum())}"
            return repr(v)
        return f"{self.name}({', '.join(f'{k}={show(v)}' for k, v in self.args.items())})"


class Script:
    def __init__(self, kind, with_ids, seed, attempt, centroids, ops):
        self.kind, self.with_ids, self.seed, self.attempt, self.C, self.ops = kind, with_ids, seed, attempt, centroids, ops
        self.dim, self.metric, self.order = shape_of(kind, with_ids, seed)

    def prefix(self, upto):
        return "\n".join(f"  {i:2d} {op}" for i, op in enumerate(self.ops[:upto + 1]))


def apply(m, op):
    """run one step on a Model -> what the call returns"""
    a = op.args
    if op.name == "add":
        return m.add(a["rows"], a.get("ids"))
    if op.name == "reserve":
        return m.reserve(a["n"])
    if op.name == "set_filter":
        return m.set_filter(a["mask"])
    if op.name == "filter_column":
        return m.filter_column(a["column"], a["op"], a["value"], a["combine"])
    if op.name in ("remove", "remove_device"):
        return m.remove(a["labels"])
    if op.name == "remove_rows":
        return m.remove_rows(a["pos"])
    if op.name == "compact":
        return m.compact()
    raise ValueError(op.name)


def _metric_lists(metric, W, C):
    """the lists of rows in plain float64: what the generator and coverage() size lists by when no oracle is at hand"""
    W, C = W.astype(np.float64), C.astype(np.float64)
    dot = W @ C.T
    if metric == 0:
        d = (W * W).sum(1)[:, None] - 2 * dot + (C * C).sum(1)[None, :]
    elif metric == 1:
        d = -dot / np.maximum(np.linalg.norm(W, axis=1)[:, None] * np.linalg.norm(C, axis=1)[None, :], 1e-30)
    else:
        d = -dot
    return np.argmin(d, axis=1) if W.shape[0] else np.empty(0, np.int64)


class _Gen:
    """one draw of a script.  The rows of list c are its centroid plus noise, list 0 being drawn several times as often as the
    others; the centroids have one norm, so that the three metrics agree on most lists"""
    P_LIST = np.array([0.44] + [0.08] * 7)

    def __init__(self, kind, with_ids, seed, attempt):
        self.kind, self.with_ids, self.seed, self.plan = kind, with_ids, seed, seed % 3
        self.dim, self.metric, self.order = shape_of(kind, with_ids, seed)
        self.rng = np.random.default_rng([KINDS.index(kind), int(with_ids), seed, attempt, 20261])
        self.scale = 20.0 if kind == "i8" else 1.0
        d = self.rng.standard_normal((NLIST, self.dim))
        self.C = (4.0 * self.scale * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
        self.m = Model(kind, self.dim, with_ids, assign=lambda w: _metric_lists(self.metric, w, self.C))
        self.ops = []
        self.next_id = 0
        self.gone_ids = np.empty(0, np.int64)  # ids of rows that compactions dropped
        self.Qbase = self._points(NQ)
        self.crossed = False                   # the IVF handle's 4096-row capacity has been left behind

    # ---- data ----
    def _points(self, n):
        c = self.rng.choice(NLIST, n, p=self.P_LIST)
        x = self.C[c] + self.rng.standard_normal((n, self.dim)) * (0.5 * self.scale)
        if self.kind == "i8":
            return np.clip(np.rint(x), -128, 127).astype(np.int8)
        return x.astype(F).astype(DTYPES[self.kind])

    def _ids(self, n):
        """distinct multiples far from the positions (as remove_cases.ids_for); now and then one of them repeats a live row's id"""
        ids = (np.arange(self.next_id, self.next_id + n, dtype=np.int64)) * 1_000_003_001 - 5_000_000_000
        self.next_id += n
        live = np.flatnonzero(self.m.live)
        if live.size and n > 2 and self.rng.random() < 0.5:
            ids[self.rng.integers(0, n)] = self.m.ids[self.rng.choice(live)]
        return ids

    # ---- emitting ----
    def emit(self, name, **args):
        op = Op(name, **args)
        before = self.m.ids[self.m.live == 0] if (name == "compact" and self.with_ids) else None
        apply(self.m, op)
        if before is not None:
            self.gone_ids = np.union1d(self.gone_ids, before)
        step = len(self.ops)
        m, rng = self.m, self.rng
        vis = m.visible()
        Q = self.Qbase.copy()
        for slot, rows in ((0, np.flatnonzero(m.live == 0)), (1, np.flatnonzero(vis)), (2, np.flatnonzero((m.live != 0) & ~vis))):
            if rows.size:  # planted: a removed row's own vector, a visible row's, a live row's that the filter hides
                Q[slot] = m.rows[rng.choice(rows)]
        op.Q = Q
        nvis = int(vis.sum())
        op.k64 = 0 < nvis < K_PAD or step % 8 == 0
        op.device = step % 2 == 1
        if step % 5 == 0 and m.ntotal:
            short = rng.integers(0, m.ntotal, (NQ, 40)).astype(np.int64)
            dead = np.flatnonzero(m.live == 0)
            if dead.size:
                short[:, :12] = dead[rng.integers(0, dead.size, (NQ, 12))]
            short[:, 13], short[:, 20] = -1, short[:, 21]
            op.short = short
        self.ops.append(op)
        return op

    def add(self, n):
        n = int(max(1, min(n, MAX_ADD, MAX_ROWS - 1 - self.m.ntotal)))
        self.emit("add", rows=self._points(n), **({"ids": self._ids(n)} if self.with_ids else {}))
        self.crossed = self.crossed or self.m.ntotal > 4096

    def room(self):
        """rows an add may bring: below MAX_ROWS, and short of the IVF capacity step while a block still has to cross it"""
        top = MAX_ROWS - 1 if (self.crossed or self.plan == 2) else 4000
        return max(0, min(MAX_ADD, top - self.m.ntotal))

    def mask(self):
        return rv.byte_mask(self.rng, self.m.ntotal, self.rng.choice([0.02, 0.1, 0.3, 0.6, 0.9, 0.97]))

    def column(self):
        """-> column, op, value: an int64 column of ten values 2^33 apart, or a float32 one; 2 % to 97 % of the rows match"""
        n, rng = self.m.ntotal, self.rng
        if rng.random() < 0.5:
            col = (rng.integers(0, 10, n).astype(np.int64) - 5) * 2 ** 33 + 5
            op = int(rng.choice(rv.OPS))
            v = int(rng.integers(1, 9))
            return col, op, (v - 5) * 2 ** 33 + 5
        col = rng.random(n, dtype=F)
        op = int(rng.choice([rv.GT, rv.GE, rv.LT, rv.LE]))
        frac = float(rng.choice([0.03, 0.2, 0.5, 0.8, 0.96]))
        return col, op, float(F(frac if op in (rv.LT, rv.LE) else 1 - frac))

    def removal(self, by_label, rows=None, junk=None, everything=False):
        """a removal set: 1 row up to 40 % of the live rows (or all of them), now and then with what the header says is ignored
        mixed in: -1, ntotal, ntotal + 5, an unknown id, a label twice, rows already removed"""
        m, rng = self.m, self.rng
        live, dead = np.flatnonzero(m.live), np.flatnonzero(m.live == 0)
        if rows is None:
            if everything or live.size == 0:
                rows = live
            else:
                frac = float(rng.choice([0.0, 0.0, 0.02, 0.1, 0.25, 0.4]))
                cnt = int(max(1, min(live.size * 0.4, round(live.size * frac) if frac else rng.integers(1, 4))))
                rows = rng.choice(live, cnt, replace=False)
        rows = np.asarray(rows, np.int64)
        vals = m.ids[rows] if (by_label and self.with_ids) else rows
        if junk if junk is not None else rng.random() < 0.35:
            extra = [-1, m.ntotal, m.ntotal + 5]
            if by_label and self.with_ids:
                extra = [-1, UNKNOWN_ID]
            if rows.size:
                extra.append(int(vals[0]))
            if dead.size:
                gone = rng.choice(dead, min(3, dead.size), replace=False)
                extra += (m.ids[gone] if (by_label and self.with_ids) else gone).tolist()
            vals = np.concatenate([vals, np.array(extra, np.int64)])
        return rng.permutation(vals).astype(np.int64)

    def remove(self, how=None, **kw):
        how = how or str(self.rng.choice(["remove", "remove_rows", "remove_device"]))
        vals = self.removal(how != "remove_rows", **kw)
        self.emit(how, **({"pos": vals} if how == "remove_rows" else {"labels": vals}))

    # ---- single operations, by weight ----
    def random_op(self):
        m, rng = self.m, self.rng
        nlive = int(np.count_nonzero(m.live))
        if nlive < 300 and self.room() > 0:
            return self.add(rng.integers(300, 1200))
        pick = rng.choice(["add", "reserve", "set_filter", "clear", "column", "remove", "compact", "remove_all"],
                          p=[0.2, 0.05, 0.14, 0.08, 0.16, 0.27, 0.08, 0.02])
        if pick == "add":
            if self.room() == 0:
                return self.emit("compact")
            return self.add(rng.choice([1, 3, 130, 700, 1500, MAX_ADD]) if rng.random() < 0.5 else rng.integers(1, MAX_ADD + 1))
        if pick == "reserve":
            top = MAX_ROWS + 3000 if self.crossed or self.plan == 2 else 4096
            n = int(rng.integers(max(1, m.ntotal // 2), top))
            self.emit("reserve", n=n)
            self.crossed = self.crossed or self.m.ivf_cap > 4096
            return None
        if pick == "set_filter":
            return self.emit("set_filter", mask=self.mask())
        if pick == "clear":
            return self.emit("set_filter", mask=None)
        if pick == "column":
            col, op, v = self.column()
            return self.emit("filter_column", column=col, op=op, value=v, combine=bool(rng.random() < 0.5))
        if pick == "remove":
            return self.remove()
        if pick == "compact":
            return self.emit("compact")
        self.remove(everything=True)           # every live row goes; an add follows at once
        return self.add(rng.integers(400, 1500))

    # ---- blocks: the states of STATES, in STATES' order ----
    def block_after_compaction(self):
        """with ids: compact, add, remove by id a row added since, beside ids of rows that left.  Without: remove by label,
        compact (the labels are renumbered), remove by the same label values"""
        m, rng = self.m, self.rng
        if self.with_ids:
            self.remove("remove", junk=False)
            self.emit("compact")
            n0 = m.ntotal
            self.add(rng.integers(5, 400))
            new = rng.choice(np.arange(n0, m.ntotal), min(3, m.ntotal - n0), replace=False)
            left = rng.choice(self.gone_ids, min(4, self.gone_ids.size), replace=False)
            self.emit(str(rng.choice(["remove", "remove_device"])), labels=rng.permutation(np.concatenate([m.ids[new], left])))
        else:
            live = np.flatnonzero(m.live)
            rows = rng.choice(live[: max(2, live.size // 2)], max(1, min(40, live.size // 8)), replace=False)
            self.emit("remove", labels=rows.astype(np.int64))
            self.emit("compact")
            self.emit("remove", labels=rows.astype(np.int64))

    def block_filter_cleared_between_compactions(self):
        self.emit("set_filter", mask=rv.byte_mask(self.rng, self.m.ntotal, 0.6))
        self.remove()
        self.emit("compact")
        self.emit("set_filter", mask=None)
        self.remove()
        self.emit("compact")

    def block_empty_under_filter(self):
        self.emit("set_filter", mask=rv.byte_mask(self.rng, self.m.ntotal, 0.5))
        self.remove(everything=True)
        self.emit("compact")
        self.add(self.rng.integers(1, 9))      # fewer visible rows than k
        self.add(self.rng.integers(600, 1500))

    def block_grow(self, filtered):
        """remove, then an add that takes both handles beyond their capacity, under a filter or without one; under a filter a
        filter_column(combine=True) and a removal follow"""
        m, rng = self.m, self.rng
        if m.ntotal < 2000:
            self.add(rng.integers(2000 - m.ntotal, 2400 - m.ntotal + 1))
        self.remove(junk=False)
        if filtered:
            self.emit("set_filter", mask=rv.byte_mask(rng, m.ntotal, 0.7))
        elif m.mask is not None:
            self.emit("set_filter", mask=None)
            self.remove(junk=False)
        need = max(m.flat_cap, m.ivf_cap) + int(rng.integers(1, 300)) - m.ntotal
        self.add(need)
        if filtered:
            col, op, v = self.column()
            self.emit("filter_column", column=col, op=op, value=v, combine=True)
            self.remove()

    def block_noop_compaction(self):
        self.remove()
        self.emit("compact")
        self.emit("compact")
        self.remove()

    def block_shared_word(self):
        """a removal at the end of the rows while ntotal is no multiple of 4, then an add: it fills the word the removal cleared"""
        m = self.m
        if m.ntotal % 4 == 0:
            self.add(int(self.rng.integers(1, 4)))
        tail = np.arange(m.ntotal - m.ntotal % 4, m.ntotal)
        self.remove("remove_rows", rows=tail[m.live[tail] != 0][:2], junk=False)
        self.add(self.rng.integers(1, 700))

    def draw(self):
        rng = self.rng
        self.add(rng.integers(1000, 1501))
        blocks = [self.block_after_compaction, self.block_filter_cleared_between_compactions, self.block_empty_under_filter,
                  self.block_noop_compaction, self.block_shared_word]
        blocks = [blocks[i] for i in rng.permutation(len(blocks))]
        if self.plan != 2:  # the one capacity step of the IVF handle: seed 0 (mod 3) leaves it without a filter, seed 1 under one
            blocks.insert(int(rng.integers(0, 3)), lambda: self.block_grow(filtered=self.plan == 1))
        for b in blocks:
            for _ in range(int(rng.integers(1, 4))):
                self.random_op()
            if self.m.ntotal == 0 or not self.m.live.any():
                self.add(rng.integers(600, 1500))
            b()
        for _ in range(2):
            self.random_op()


def coverage(s, lists=None):
    """replay `s` on a fresh Model -> dict: ops (names that occurred), states (of STATES), grow (the (handle, filtered) pairs of adds
    that grew a handle holding removed rows), compact ({"filter", "no filter", "nothing removed", "empty then add"}), and per check
    nvisible, ntotal, padded (0 < nvisible < the largest k searched) and the longest visible list.  lists: step -> the lists of the rows
    after that step (the oracle's); None: plain float64 ones"""
    m = Model(s.kind, s.dim, s.with_ids, assign=lambda w: _metric_lists(s.metric, w, s.C))
    out = {"ops": set(), "states": set(), "grow": set(), "compact": set(), "nvisible": [], "padded": [], "longest": [], "ntotal": []}
    hist = []                        # (name, facts) of the steps so far
    gone_ids = np.empty(0, np.int64)
    since = None                     # ntotal after the last compaction that dropped rows: the rows from there on came later
    old_label_sets = []              # label sets of removals before the last renumbering compaction
    cur_label_sets = []
    removed_once = False
    for step, op in enumerate(s.ops):
        a = op.args
        nt, nlive, ndead, _ = m.counts()
        had_mask = m.mask is not None
        fact = {"ndead": ndead, "mask": had_mask, "nlive": nlive}
        name = op.name
        out["ops"].add(name)
        if name == "set_filter":
            out["ops"].add("set_filter(None)" if a["mask"] is None else "set_filter(mask)")
        if name == "filter_column":
            out["ops"].add(f"filter_column {a['column'].dtype} combine={a['combine']}")
        if name == "add" and nt % 4 and (m.live[nt - nt % 4:] == 0).any():
            out["states"].add(STATES[6])
        if name in ("remove", "remove_device") and s.with_ids:
            lab = a["labels"]
            fresh_rows = np.flatnonzero((m.live != 0) & np.isin(m.ids, lab))
            if since is not None and (fresh_rows >= since).any() and np.isin(lab, gone_ids).any():
                out["states"].add(STATES[0])
        if name == "compact" and s.with_ids:
            gone_ids = np.union1d(gone_ids, m.ids[m.live == 0])
        ret = apply(m, op)
        fact["ret"] = ret if not isinstance(ret, np.ndarray) else None
        if name in ("remove", "remove_rows", "remove_device") and ret:
            removed_once = True
        if name == "remove" and not s.with_ids:
            key = tuple(sorted(a["labels"].tolist()))
            if ret and key in old_label_sets:
                out["states"].add(STATES[4])
            cur_label_sets.append(key)
        if name == "compact":
            if ndead:
                out["compact"].add("filter" if had_mask else "no filter")
                since = m.ntotal
                old_label_sets, cur_label_sets = cur_label_sets, []
            else:
                out["compact"].add("nothing removed")
                if removed_once and hist and hist[-1][0] == "compact" and hist[-1][1]["ndead"]:
                    out["states"].add(STATES[5])
        if name == "add":
            for handle, grew in zip(("flat", "ivf"), m.grew):
                if grew and ndead:
                    out["grow"].add((handle, had_mask))
            if hist and hist[-1][0] == "compact" and hist[-1][1]["ndead"] and hist[-1][1]["nlive"] == 0:
                out["compact"].add("empty then add")
                if hist[-1][1]["mask"]:
                    out["states"].add(STATES[2])
        names = [h[0] for h in hist[-5:]] + [name]
        facts = [h[1] for h in hist[-5:]] + [fact]
        rm = ("remove", "remove_rows", "remove_device")
        # compact under a filter, set_filter(None), a removal that removes, compact
        if (len(names) >= 4 and names[-4] == "compact" and facts[-4]["mask"] and facts[-4]["ndead"] and names[-3] == "set_filter"
                and not facts[-2]["mask"] and names[-2] in rm and facts[-2]["ret"] and name == "compact"):
            out["states"].add(STATES[1])
        # a removal that removes, an add that grows both handles under a filter, filter_column(combine=True), a removal
        if (len(names) >= 4 and names[-4] in rm + ("set_filter",) and names[-3] == "add" and facts[-3].get("grew") == (True, True)
                and facts[-3]["mask"] and facts[-3]["ndead"] and names[-2] == "filter_column" and s.ops[step - 1].args["combine"]
                and name in rm and ret):
            out["states"].add(STATES[3])
        if name in ("add", "reserve"):
            fact["grew"] = m.grew
        hist.append((name, fact))
        vis = m.visible()
        nvis = int(vis.sum())
        L = m.lists if lists is None else lists[step]
        out["nvisible"].append(nvis)
        out["ntotal"].append(m.ntotal)
        out["padded"].append(0 < nvis < (K_PAD if op.k64 else KS[-1]))
        out["longest"].append(int(np.bincount(L[vis], minlength=NLIST).max()) if nvis else 0)
    return out


def missing(s, cov):
    """what `s` lacks of what is asked of every script and of its seed -> list of texts (empty: the script stands)"""
    out = []
    if not 30 <= len(s.ops) <= 60:
        out.append(f"{len(s.ops)} operations")
    lack = (set(MUTATING) | {"set_filter(None)", "set_filter(mask)"}) - cov["ops"]
    if lack:
        out.append(f"operations {sorted(lack)}")
    want = set(STATES) - {STATES[3], NO_IDS_ONLY if s.with_ids else IDS_ONLY}
    if s.seed % 3 == 1:
        want.add(STATES[3])
    out += [f"state: {x}" for x in sorted(want - cov["states"])]
    if s.seed % 3 == 0 and not {("flat", False), ("ivf", False)} <= cov["grow"]:
        out.append("an add that grows both handles over removed rows, no filter")
    if s.seed % 3 == 1 and not {("flat", True), ("ivf", True)} <= cov["grow"]:
        out.append("an add that grows both handles over removed rows, under a filter")
    lack = {"filter", "no filter", "nothing removed", "empty then add"} - cov["compact"]
    if lack:
        out.append(f"compactions {sorted(lack)}")
    n = len(cov["nvisible"])
    if sum(v < 10 for v in cov["nvisible"]) * 4 > n:
        out.append("more than a quarter of the checks see fewer than 10 rows")
    if not any(cov["padded"]):
        out.append("no check with 0 < nvisible < k")
    if max(cov["longest"]) <= 128:
        out.append("no visible list beyond the 128-row tile")
    if max(cov["ntotal"]) >= MAX_ROWS:
        out.append("too many rows")
    return out


@functools.lru_cache(maxsize=None)
def script(seed, kind, with_ids):
    """the script of (seed, kind, with_ids): the first draw that lacks nothing.  Deterministic; never written to"""
    for attempt in range(400):
        g = _Gen(kind, with_ids, seed, attempt)
        try:
            g.draw()
        except (ValueError, IndexError):  # a block that does not apply to the state it met (nothing left to choose from)
            continue
        s = Script(kind, with_ids, seed, attempt, g.C, g.ops)
        if not missing(s, coverage(s)):
            for op in s.ops:
                for v in list(op.args.values()) + [op.Q, op.short]:
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
            s.C.setflags(write=False)
            return s
    raise RuntimeError(f"no script for seed {seed} {kind} ids {with_ids} in 400 draws")
