"""An add to a code IVF handle (IVF-SQ8, IVF-BQ, IVF-PQ plain and residual) that crosses piece_rows(dims), the rows the shared add
(lb_ivf_host.h: ivf_add) assigns and encodes at a time: the one path of it that the other tests, whose adds are a single piece, do
not reach.  The smallest shape that crosses it is dims = LB_MAX_DIM = 8192, where piece_rows is 8192, and 8192 + 129 rows in ONE
add; about 270 MB of f32, so a module builds the case once (a module-scoped fixture) and lets it go.

What is asserted: the handle filled by that one add, from host memory or through add_device, equals bit for bit a handle of the
same kind filled with the same rows and ids by adds of at most 4096 rows each, the single-piece path that the handles' own tests
hold to the oracle; and its assignments equal the CPU oracle's coarse assignment."""
import numpy as np

F = np.float32
DIMS = 8192          # LB_MAX_DIM: piece_rows(DIMS) == 8192
N = 8192 + 129       # a full piece and a ragged one
NLIST = 4
SMALL = 4096         # rows per add of the handle compared against
NQ, K, NPROBE = 5, 10, 2
assert (64 << 20) // DIMS == 8192 < N


def case(seed=20):
    """-> rows [N, DIMS] uniform in [-0.5, 0.5), ids, centroids (NLIST of the rows), queries"""
    rng = np.random.default_rng(seed)
    X = rng.random((N, DIMS), dtype=F)
    X -= F(0.5)
    ids = (np.int64(1) << 40) + rng.permutation(N).astype(np.int64) * 3
    C_ = X[np.sort(rng.permutation(N)[:NLIST])].copy()
    Q = rng.random((NQ, DIMS), dtype=F) - F(0.5)
    return X, ids, C_, Q


def fill(h, X, ids, step, device=False):
    """rows X with ids into h by adds of at most `step` rows, from host memory or through add_device"""
    if device:
        import torch
        dX, dI = torch.from_numpy(X).cuda(), torch.from_numpy(ids).cuda()
        torch.cuda.synchronize()
    for r0 in range(0, X.shape[0], step):
        cnt = min(step, X.shape[0] - r0)
        if device:
            h.add_device(cnt, dX[r0:].data_ptr(), dI[r0:].data_ptr())
        else:
            h.add(X[r0:r0 + cnt], ids[r0:r0 + cnt])
    return h


def snapshot(h, Q):
    """what is compared between two handles: codes, assignments, list sizes and a search"""
    lab, dist = h.search(Q, K, NPROBE)
    return {"ntotal": h.ntotal, "codes": h.codes(), "assignments": h.assignments(), "list_sizes": h.list_sizes(), "labels": lab, "dist": dist}


def assert_same_handle(got, want, ctx=""):
    assert got["ntotal"] == want["ntotal"] == N, (got["ntotal"], want["ntotal"], ctx)
    for key in ("codes", "assignments", "list_sizes", "labels", "dist"):
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (key, ctx)
        assert np.array_equal(got[key], want[key]), f"{key} differ {ctx}: {np.argwhere(got[key] != want[key])[:5]}"


def reference(new_handle, X, ids, Q):
    """the snapshot of a fresh handle filled by adds of at most SMALL rows each"""
    h = fill(new_handle(), X, ids, SMALL)
    try:
        return snapshot(h, Q)
    finally:
        h.Close()


def check_one_add(new_handle, X, ids, Q, want, lists, device):
    """a fresh handle filled by ONE add of all N rows against `want` (reference()) and the oracle's assignment `lists`"""
    h = fill(new_handle(), X, ids, N, device)
    try:
        got = snapshot(h, Q)
    finally:
        h.Close()
    ctx = "add_device" if device else "add"
    assert_same_handle(got, want, ctx)
    assert np.array_equal(got["assignments"], lists), f"assignments differ from the oracle's ({ctx}): {np.flatnonzero(got['assignments'] != lists)[:5]}"
    assert (got["labels"] >= 0).all() and np.isin(got["labels"], ids).all(), ctx  # (every query finds K of the ids given)
