"""Long result lists (k = 600 .. LB_MAX_K) on large corpora: the call shape of ArrowHNSW.SearchHybrid, which asks the GPU for
min(10 k, Len) candidates -- k = 100 becomes a search for 1000.

At this size the schedule differs from k <= 512: the fp16 routes keep 4096 candidates, which no sampled threshold reaches (the
classic bootstrap and growing chunks run over the fp16 image); the f32 routes get one sampled span of about 2.3M rows; the
finish launch holds at most 2 k members (smax = 4096 at k = 2048), and a query whose members overflow it is redone on another
route.  Every one of these routes is exact: each list here is compared bit for bit (labels and distances, -1 / FLT_MAX
padding) with the same search on another route and with the oracle on a subsample.

Each test prints one line per search: route (kind * 10 + operand form) and the queries that needed the exact-scan fallback."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import i8_oracle as io
from tests.gpu_util import assert_same, gpu_or_skip, oracle_topk_rows_parallel

pytestmark = pytest.mark.gpu

F = np.float32
L2, COS, DOT = 0, 1, 2
N, D = 1_000_000, 768
BATCHES = (1, 4, 8, 16, 64, 256, 1024)
LB_MAX_K = 2048


def _index(metric, dtype=0, dim=D):
    from longbow_amd import gpu
    return gpu.NewIndexWithConfig(gpu.GPUConfig(DeviceID=0, Dimension=dim, Metric=metric, DataType=dtype))


def _search(torch, idx, d_q, nq, k):
    """one search_device call on the first nq rows of the device tensor d_q -> host (labels, distances, route, fallbacks)"""
    dd = torch.empty((nq, k), device="cuda")
    dl = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    idx.search_device(nq, d_q.data_ptr(), k, dd.data_ptr(), dl.data_ptr())
    route = int(idx._lib.lb_gpu_index_last_route(idx._h))
    return dl.cpu().numpy(), dd.cpu().numpy(), route, idx.last_fallbacks


def _report(tag, route, fb):
    print(f"[long-lists] {tag}: route {route} fallbacks {fb}", flush=True)


@pytest.fixture(scope="class")
def uniform_1m():
    """1M x 768 uniform f32 rows and 1024 queries filled on the device (the bench's data), plus the host copy the oracle reads"""
    gpu_or_skip()
    torch = pytest.importorskip("torch")
    from longbow_amd import _lib
    lib = _lib.load()
    X = torch.empty((N, D), device="cuda")
    Q = torch.empty((1024, D), device="cuda")
    assert lib.lb_gpu_fill_uniform_device(0, X.data_ptr(), X.numel(), 12345, 0, None) == 0
    assert lib.lb_gpu_fill_uniform_device(0, Q.data_ptr(), Q.numel(), 42, 0, None) == 0
    ns = {"torch": torch, "X": X, "Q": Q, "Xh": X.cpu().numpy(), "Qh": Q.cpu().numpy()}
    yield ns
    ns.clear()
    del X, Q
    torch.cuda.empty_cache()


class TestUniform1M:
    # ----------------------------------------------------------------------------------------------------------------------
    # a. every batch form of the finish launch at k = 600 / 1000 / 2048, three candidate modes, prefixes and the oracle
    # ----------------------------------------------------------------------------------------------------------------------
    @pytest.mark.parametrize("metric", [L2, COS, DOT])
    def test_routes_agree_and_match_oracle(self, oracle, uniform_1m, metric):
        torch, X, Q, Xh, Qh = (uniform_1m[s] for s in ("torch", "X", "Q", "Xh", "Qh"))
        idx = _index(metric)
        over = []  # (ctx, fallbacks) beyond the bound: reported after every exactness check has run
        try:
            idx.reserve(N)
            idx.add_device(N, X.data_ptr())
            giveups = idx.fused_giveups
            sub = [0, 3, 9, 15, 200, 1023]  # queries of every batch size's prefix and the largest batch's last one
            want = {q: oracle_topk_rows_parallel(oracle, metric, Qh[q], Xh, LB_MAX_K, nthreads=16) for q in sub}
            for k in (600, 1000, 2048):
                ref = None
                for mode in ("auto", "strict", "image off"):
                    if mode == "strict":
                        idx.set_candidate_mode(0)
                    elif mode == "image off":
                        idx.set_candidate_mode(3)
                        idx.set_f16_image(0)
                    for B in sorted(BATCHES, reverse=True):
                        lab, dist, route, fb = _search(torch, idx, Q, B, k)
                        ctx = f"metric {metric} k {k} B {B} {mode}"
                        _report(ctx, route, fb)
                        ctx += f": route {route} fallbacks {fb}"
                        if ref is None:
                            ref = (lab, dist)  # AUTO over 1024 queries: every other search is a prefix of it
                        assert_same(lab, dist, ref[0][:B], ref[1][:B], ctx)
                        assert idx.fused_giveups == giveups, ctx
                        if B >= 16:
                            assert route // 10 != 0, ctx
                        if B >= 64 and fb > B // 20:
                            over.append(ctx)
                    idx.set_f16_image(1)
                for q in sub:
                    assert_same(ref[0][q], ref[1][q], want[q][0][:k], want[q][1][:k], f"metric {metric} k {k} oracle query {q}")
            assert not over, f"more than B // 20 queries fell back to the exact scan: {over}"
        finally:
            idx.Close()

    # ----------------------------------------------------------------------------------------------------------------------
    # c. filtered views at large k: a row list over the fp16 image, the per-row test over f32 rows, views of k - 1 / k / k + 1
    # rows (padding, the one-row boundary), user ids
    # ----------------------------------------------------------------------------------------------------------------------
    def test_filtered_views(self, oracle, uniform_1m):
        torch, X, Q, Xh, Qh = (uniform_1m[s] for s in ("torch", "X", "Q", "Xh", "Qh"))
        rng = np.random.default_rng(11)
        B = 256
        views = [("10 %", rng.random(N) < 0.10, 1000, False),
                 ("97 %", rng.random(N) < 0.97, 1000, False)]
        for nv in (LB_MAX_K - 1, LB_MAX_K, LB_MAX_K + 1):
            m = np.zeros(N, bool)
            m[rng.choice(N, nv, replace=False)] = True
            views.append((f"{nv} rows", m, LB_MAX_K, nv == LB_MAX_K + 1))
        views.append(("10 % with ids", views[0][1], 1000, True))
        ids = (np.int64(7) << 40) + rng.permutation(N).astype(np.int64) * 3  # distinct, unordered, far from the row numbers
        plain, with_ids = _index(DOT), _index(DOT)
        try:
            plain.add_device(N, X.data_ptr())
            d_ids = torch.from_numpy(ids).cuda()
            with_ids.add_device(N, X.data_ptr(), d_ids.data_ptr())
            del d_ids
            sub = np.arange(0, B, 32)
            for name, mask, k, use_ids in views:
                idx = with_ids if use_ids else plain
                idx.set_filter(mask.astype(np.uint8))
                lab, dist, route, fb = _search(torch, idx, Q, B, k)
                _report(f"view {name} k {k}", route, fb)
                idx.set_candidate_mode(0)
                lab0, dist0, route0, fb0 = _search(torch, idx, Q, B, k)
                idx.set_candidate_mode(3)
                _report(f"view {name} k {k} strict", route0, fb0)
                ctx = f"view {name} k {k}: route {route} fallbacks {fb}, strict route {route0} fallbacks {fb0}"
                assert_same(lab, dist, lab0, dist0, ctx + " AUTO = strict")
                oi, od = oracle.search_batch(DOT, Qh[sub], Xh, k, mask=mask, ids=ids if use_ids else None, nthreads=16)
                assert_same(lab[sub], dist[sub], oi, od, ctx + " oracle")
                nv = int(mask.sum())
                if nv < k:  # padding: every visible row, then -1 / FLT_MAX
                    assert np.all(lab[:, nv:] == -1) and np.all(dist[:, nv:] == np.finfo(F).max), ctx
                    assert np.all(lab[:, :nv] >= 0), ctx
                idx.set_filter(None)
        finally:
            plain.Close()
            with_ids.Close()

    # ----------------------------------------------------------------------------------------------------------------------
    # d. the GPU -> HNSW hand-off as Longbow issues it: min(10 k, Len) candidates, tombstoned ids dropped, first k kept
    # ----------------------------------------------------------------------------------------------------------------------
    def test_hybrid_handoff(self, oracle, uniform_1m):
        from longbow_amd import hybrid
        from longbow_amd.gpu import LongbowGPUError
        X, Xh, Qh = uniform_1m["X"], uniform_1m["Xh"], uniform_1m["Qh"]
        live = np.random.default_rng(12).random(N) >= 0.30
        idx = _index(L2)
        try:
            idx.add_device(N, X.data_ptr())
            got = {}
            for k in (100, 204):  # 1000 and 2040 candidates
                for q in (5, 77, 500):
                    ids, dist = hybrid.search_hybrid_candidates(idx, Qh[q], k, is_live=lambda i: live[i])
                    ol, od = oracle_topk_rows_parallel(oracle, L2, Qh[q], Xh, 10 * k, nthreads=16)
                    keep = live[ol]
                    assert_same(ids, dist, ol[keep][:k], od[keep][:k], f"k {k} query {q}")
                    got[(k, q)] = (ids, dist)
            with pytest.raises(LongbowGPUError):  # 2050 candidates > LB_MAX_K: refused, nothing searched
                hybrid.search_hybrid_candidates(idx, Qh[5], 205, is_live=lambda i: live[i])
            ids, dist = hybrid.search_hybrid_candidates(idx, Qh[5], 204, is_live=lambda i: live[i])
            assert_same(ids, dist, *got[(204, 5)], "after the refused search")
        finally:
            idx.Close()

    # ----------------------------------------------------------------------------------------------------------------------
    # e. concurrent single-query searches at k = 1000 answered by combined batches
    # ----------------------------------------------------------------------------------------------------------------------
    def test_combined_single_searches(self, uniform_1m):
        X, Qh = uniform_1m["X"], uniform_1m["Qh"]
        T, PER, k = 16, 3, 1000
        idx = _index(COS)
        try:
            idx.add_device(N, X.data_ptr())
            idx.set_search_combining(False)
            solo = [idx.Search(Qh[i], k) for i in range(T * PER)]
            idx.set_search_combining(True)
            out = [None] * (T * PER)
            errors = []
            start = threading.Barrier(T)

            def work(t):
                try:
                    start.wait()
                    for j in range(PER):
                        out[t * PER + j] = idx.Search(Qh[t * PER + j], k)
                except Exception as e:  # noqa: BLE001 (reported below)
                    errors.append(repr(e))

            ths = [threading.Thread(target=work, args=(t,)) for t in range(T)]
            [t.start() for t in ths]
            [t.join() for t in ths]
            assert not errors, errors[:5]
            for i in range(T * PER):
                assert_same(out[i][0], out[i][1], solo[i][0], solo[i][1], f"caller {i}")
            batches, requests = idx.combining_stats
            assert batches > 0 and requests >= 2 * batches, (batches, requests)
        finally:
            idx.Close()


# --------------------------------------------------------------------------------------------------------------------------
# b. the edges of the sampled span: strict mode (kept candidates = kc), 128 dimensions, k = 1000.  The corpus sizes come from
# the plan itself: the largest one a single span covers, and the smallest one whose span ends short and leaves the growing
# chunks a tail.  Queries are exact hits on the rows at either side of each boundary, so a schedule that drops or repeats a
# boundary row changes a list.
# --------------------------------------------------------------------------------------------------------------------------
def _plan(diag, n, keep, cap, count_max):
    out = (C.c_longlong * 4)()
    diag.lb_debug_sample_plan(n, keep, cap, count_max, out)
    return bool(out[0]), int(out[1])


def _covers(diag, n, keep, cap, count_max):
    on, span = _plan(diag, n, keep, cap, count_max)
    return on and span >= n


@pytest.mark.parametrize("metric", [L2, COS])
def test_sampled_span_edges(oracle, metric):
    gpu_or_skip()
    torch = pytest.importorskip("torch")
    from longbow_amd import _lib
    diag = _lib.load_diag()  # (host-only plan hooks; the index itself runs on the product library)
    k, dim = 1000, 128
    kc, cap = C.c_int(0), C.c_uint(0)
    diag.lb_debug_cand_geometry(k, C.byref(kc), C.byref(cap))
    kc, cap = kc.value, cap.value
    # batched searches sample up to 8192 rows with kc kept; the 1-query scan samples 4096 with k kept (run_scan_path)
    batched, scan = (kc, cap, 8192), (k, cap, 4096)
    lo, hi = 1 << 20, 1 << 26  # (small views do not get a plan at all: the search starts from a size one span covers)
    assert _covers(diag, lo, *batched) and not _covers(diag, hi, *batched)
    while hi - lo > 1:  # the largest n one span covers (beyond it the span is capped by the list capacity, whatever n is)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _covers(diag, mid, *batched) else (lo, mid)
    n_cover = lo
    n_short = next(n for n in range(n_cover + 1, n_cover + 4097) if _plan(diag, n, *batched)[0])
    on, span = _plan(diag, n_short, *batched)
    # the plans this test is about: one span over n_cover rows; over n_short rows a span that ends a few rows short
    assert _covers(diag, n_cover, *batched)
    assert on and span < n_short and n_short - span <= 4096, (n_cover, n_short, span)
    edges = {n_cover - 1, span - 1, span, n_short - 1}
    for n in (n_cover, n_short):
        on_s, span_s = _plan(diag, n, *scan)
        if on_s and span_s < n:
            edges |= {span_s - 1, span_s}
    edges = sorted(edges)
    rng = np.random.default_rng(13 + metric)
    X = rng.random((n_short, dim), dtype=F)
    Qh = rng.random((256, dim), dtype=F)
    Qh[:len(edges)] = X[edges]  # exact hits on the boundary rows
    Qh[len(edges):2 * len(edges)] = X[edges] + F(1e-3)  # near hits: the boundary row and its neighbours in one list
    Q = torch.from_numpy(Qh).cuda()
    idx = _index(metric, dim=dim)
    try:
        idx.set_candidate_mode(0)
        idx.reserve(n_short)
        idx.Add(None, X[:n_cover])
        giveups = idx.fused_giveups
        for n in (n_cover, n_short):
            if n == n_short:
                idx.Add(None, X[n_cover:])
            assert idx.ntotal == n
            picks = [q for q in range(2 * len(edges))] + [100, 255]
            oi, od = oracle.search_batch(metric, Qh[picks], X[:n], k, nthreads=16)
            want = dict(zip(picks, zip(oi, od)))
            full = None
            for B in (256, 16, 1):
                if B == 1:  # one query per call: every planted query and two others
                    for q in picks:
                        lab, dist, route, fb = _search(torch, idx, Q[q:q + 1], 1, k)
                        _report(f"span edges metric {metric} n {n} B 1 query {q}", route, fb)
                        assert_same(lab[0], dist[0], *want[q], f"n {n} B 1 query {q}: route {route} fallbacks {fb}")
                    continue
                lab, dist, route, fb = _search(torch, idx, Q, B, k)
                ctx = f"span edges metric {metric} n {n} (span {span if n == n_short else n}) B {B}"
                _report(ctx, route, fb)
                ctx += f": route {route} fallbacks {fb}"
                assert idx.fused_giveups == giveups, ctx
                if full is None:
                    full = (lab, dist)
                assert_same(lab, dist, full[0][:B], full[1][:B], ctx + " prefix")
                for q in picks:
                    if q < B:
                        assert_same(lab[q], dist[q], *want[q], f"{ctx} query {q}")
            for j, e in enumerate(edges):  # the planted rows are where they should be
                if e < n:
                    assert full[0][j][0] == e, (n, e, full[0][j][:3])
    finally:
        idx.Close()


# --------------------------------------------------------------------------------------------------------------------------
# f. fp16 index, 1M x 768 standard-normal rows: lists equal an f32 index's over the widened rows (the centred L2 image over
# fp16 rows included), every query
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, COS, DOT])
def test_f16_index_long_lists(oracle, metric):
    gpu_or_skip()
    torch = pytest.importorskip("torch")
    from longbow_amd.gpu import DataType
    g = torch.Generator(device="cuda").manual_seed(21 + metric)
    Xh16 = torch.randn((N, D), generator=g, device="cuda").half()
    Qh16 = torch.randn((256, D), generator=g, device="cuda").half()
    Xf, Qf = Xh16.float(), Qh16.float()
    f16, f32 = _index(metric, DataType.Float16), _index(metric)
    f32.set_order(oc.UNROLL4)  # (an fp16 index sums in the reference F16 functions' 4-accumulator order)
    try:
        f16.add_device(N, Xh16.data_ptr())
        f32.add_device(N, Xf.data_ptr())
        del Xh16
        assert f16.f16_image_bytes > 0
        giveups = f16.fused_giveups
        Xhost, Qhost = Xf.cpu().numpy(), Qf.cpu().numpy()
        del Xf
        sub = (0, 9, 15, 255)
        want = {q: oracle_topk_rows_parallel(oracle, metric, Qhost[q], Xhost, LB_MAX_K, nthreads=16, order=oc.UNROLL4)
                for q in sub}
        for k in (10, 1000, 2048):
            for B in (256, 16, 1):
                lab, dist, route, fb = _search(torch, f16, Qh16, B, k)
                ctx = f"fp16 metric {metric} k {k} B {B}"
                _report(ctx, route, fb)
                lab32, dist32, route32, fb32 = _search(torch, f32, Qf, B, k)
                _report(ctx + " (f32 index)", route32, fb32)
                ctx += f": route {route} fallbacks {fb}, f32 index route {route32} fallbacks {fb32}"
                assert_same(lab, dist, lab32, dist32, ctx)
                assert f16.fused_giveups == giveups, ctx
                for q in sub:
                    if q < B:
                        assert_same(lab[q], dist[q], want[q][0][:k], want[q][1][:k], f"{ctx} oracle query {q}")
    finally:
        f16.Close()
        f32.Close()


# --------------------------------------------------------------------------------------------------------------------------
# g. int8 index, 1M x 768: keep = k gets a sampled span over the corpus, so the i8 MFMA pass serves k = 1000 and 2048
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, DOT])
def test_i8_index_long_lists(metric):
    gpu_or_skip()
    torch = pytest.importorskip("torch")
    from longbow_amd.gpu import DataType
    g = torch.Generator(device="cuda").manual_seed(31 + metric)
    X = torch.randint(-128, 128, (N, D), generator=g, device="cuda", dtype=torch.int8)
    Q = torch.randint(-128, 128, (128, D), generator=g, device="cuda", dtype=torch.int8)
    idx = _index(metric, DataType.Int8)
    try:
        idx.add_device(N, X.data_ptr())
        Xh, Qh = X.cpu().numpy(), Q.cpu().numpy()
        del X
        sub = np.array([0, 7, 15, 127])
        oi, od = io.search(metric, Qh[sub], Xh, LB_MAX_K)
        for k in (1000, 2048):
            for B in (128, 16):
                lab, dist, route, fb = _search(torch, idx, Q, B, k)
                ctx = f"int8 metric {metric} k {k} B {B}"
                _report(ctx, route, fb)
                ctx += f": route {route} fallbacks {fb}"
                assert route == 81, ctx  # the i8 MFMA pass: a build that silently scans fails here
                for j, q in enumerate(sub):
                    if q < B:
                        assert_same(lab[q], dist[q], oi[j][:k], od[j][:k], f"{ctx} oracle query {q}")
    finally:
        idx.Close()


# --------------------------------------------------------------------------------------------------------------------------
# Small low-dimensional corpora, k = 600 .. LB_MAX_K, one query and a batch, against the oracle (every query)
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(30000, 32), (120000, 64)])
@pytest.mark.parametrize("metric", [L2, COS])
def test_small_corpora_long_lists(oracle, n, dim, metric):
    gpu_or_skip()
    rng = np.random.default_rng(5)
    X = rng.random((n, dim), dtype=F)
    Q = rng.random((40, dim), dtype=F)
    idx = _index(metric, dim=dim)
    try:
        idx.Add(None, X)
        for k in (600, 1024, 2048):
            for nq in (1, 40):
                lab, dist = idx.SearchBatch(Q[:nq], k)
                oi, od = oracle.search_batch(metric, Q[:nq], X, k, nthreads=16)
                assert_same(lab, dist, oi, od, f"n {n} dim {dim} metric {metric} k {k} nq {nq}: fallbacks {idx.last_fallbacks}")
    finally:
        idx.Close()
