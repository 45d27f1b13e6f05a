// index_search.hip -- searching an index: the workspace pool, the exact-scan driver, route choice and the batched-search driver,
// the host-pointer staging and combining path, the view of a call that brings its own row bitmap (build_call_view; kernels in
// kernels_index_call.hip), and every lb_gpu_index_search* entry point of include/longbow_gpu.h.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_host.h"
#include "lb_index.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace lb;

namespace lb { void read_fused_probe(unsigned long long out[8], bool reset); void read_finish_probe(unsigned long long out[8], bool reset); }

constexpr int kScanMaxQ = 8;          // queries per scan launch (register accumulators)
constexpr int kGemmMinQ = 17;         // below this the exact scan path is used for everything
constexpr int kMaxBatch = 4096;       // queries per internal batch (workspace sizing)
constexpr int kFinishSplitMaxQ = 128;     // largest batch the finish launch serves with several workgroups per query
constexpr uint32_t kFinishSmaxMax = 4096; // most members (rows re-ranked exactly) a query may have

namespace {
// the test hooks' switches, with their lb_debug_* setters at the end of this file.  The first two are read by every build
// (sample_plan, run_batch) and keep their defaults in the product library; the other three exist in the diagnostic build only
std::atomic<int> g_sample_tau{1}; // test hook (diagnostic build): 0 = the classic bootstrap schedule only
std::atomic<int> g_fused_fail_next{0}; // test hook: treat the next fused launch as one whose waits gave up
#ifdef LB_DIAG
std::atomic<int> g_tin_withhold_next{0}; // test hook (diagnostic build): the next TAUIN launch's thresholds never come out
std::atomic<int> g_last_route{0}; // diagnostic build: kind * 10 + split of the last batched search's route
std::atomic<int> g_search_fail_next{0}; // test hook (diagnostic build): the next search on this process fails with LB_ERR_INTERNAL
#endif
} // namespace

// candidate-list geometry for a request of k
void cand_geometry(int k, int &kc, uint32_t &cap)
{
    int want = std::max(2 * k, k + 32);
    kc = (int)next_pow2_host((uint32_t)std::max(want, 64));
    cap = std::max<uint32_t>(8192u, 4u * (uint32_t)kc);
    // (from 1024 candidates -- k beyond 240 -- the fp16 routes keep 2048 per query: with 8192-entry lists that is a quarter of the
    // capacity, the sampled span ends short of the corpus and the rest runs the classic schedule -- 1M x 768, k = 300: 0.71 ms a
    // query where k = 100 takes 0.29)
    if (kc >= 1024) cap = std::max<uint32_t>(cap, 16384u);
}

std::unique_ptr<Workspace> acquire_ws(lb_gpu_index *h, int nq, uint32_t cap)
{
    {
        std::lock_guard<std::mutex> g(h->ws_mu);
        size_t best = (size_t)-1;
        for (size_t i = 0; i < h->ws_free.size(); i++)
            if (h->ws_free[i]->nq_cap >= nq && h->ws_free[i]->cap == cap &&
                (best == (size_t)-1 || h->ws_free[i]->nq_cap < h->ws_free[best]->nq_cap))
                best = i;
        if (best != (size_t)-1) {
            auto w = std::move(h->ws_free[best]);
            h->ws_free.erase(h->ws_free.begin() + (long)best);
            return w;
        }
    }
    auto w = std::make_unique<Workspace>();
    w->device = h->device;
    w->nq_cap = (int)next_pow2_host((uint32_t)std::max(nq, 8)); // nearby batch sizes share a workspace
    w->cap = cap;
    w->cs.cap = cap;
    LB_HIP(hipStreamCreateWithFlags(&w->stream.h, hipStreamNonBlocking));
    const size_t nqc = (size_t)w->nq_cap;
    w->d_lists.alloc(nqc * cap);
    w->d_cnt.alloc(nqc);
    w->d_tau.alloc(nqc);
    w->d_flags.alloc(nqc);
    w->d_done.alloc(nqc);
    LB_HIP(hipMemset(w->d_done.get(), 0, nqc * sizeof(uint32_t)));
    w->d_xcnt.alloc(nqc);
    LB_HIP(hipMemset(w->d_xcnt.get(), 0, nqc * sizeof(uint32_t)));
    w->d_xscratch.alloc(finish_scratch_bytes(kFinishSplitMaxQ, kFinishSmaxMax));
    w->d_fsync.alloc(1 + nqc);
    LB_HIP(hipMemset(w->d_fsync.get(), 0, (1 + nqc) * sizeof(uint32_t)));
    LB_HIP(hipMemset(w->d_flags.get(), 0, nqc * sizeof(uint32_t)));
    w->h_fail.alloc(1);
    *w->h_fail.get() = 0;
    w->d_stripes.alloc((size_t)kScanMaxQ * LB_STRIPES * LB_STRIPE_PAD);
    w->cs.lists = w->d_lists.get();
    w->cs.cnt = w->d_cnt.get();
    w->cs.tau = w->d_tau.get();
    w->cs.flags = w->d_flags.get();
    w->cs.stripes = w->d_stripes.get();
    w->d_qna.alloc(nqc);
    w->d_qsel.alloc(nqc);
    w->d_iota.alloc(nqc);
    {
        std::vector<int> iota(nqc);
        for (int i = 0; i < w->nq_cap; i++) iota[(size_t)i] = i;
        LB_HIP(hipMemcpy(w->d_iota.get(), iota.data(), iota.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    w->d_smap.alloc(cap);
    w->h_flags.alloc(nqc);
    w->h_qsel.alloc(nqc);
    return w;
}

void release_ws(lb_gpu_index *h, std::unique_ptr<Workspace> w)
{
    std::unique_ptr<Workspace> drop; // (freed outside the lock: hipFree synchronises the device)
    {
        std::lock_guard<std::mutex> g(h->ws_mu);
        if (h->ws_free.size() < 8) {
            h->ws_free.push_back(std::move(w));
            return;
        }
        // pool full: keep the LARGER workspaces.  (A pool that dropped the newcomer instead re-allocated the workspace of
        // every batch size beyond the first eight on every call: +1.4 ms per search, tools/route_grid.py.)
        size_t smallest = 0;
        for (size_t i = 1; i < h->ws_free.size(); i++)
            if (h->ws_free[i]->nq_cap < h->ws_free[smallest]->nq_cap) smallest = i;
        if (h->ws_free[smallest]->nq_cap < w->nq_cap) {
            drop = std::move(h->ws_free[smallest]);
            h->ws_free[smallest] = std::move(w);
        } else {
            drop = std::move(w);
        }
    }
}

namespace {

struct ProfScope {
    Workspace *w;
    hipStream_t s;
    bool on;
    size_t idx = 0;
    ProfScope(Workspace *w_, hipStream_t s_, bool on_, int cls) : w(w_), s(s_), on(on_)
    {
        if (!on) return;
        if (w->ev_used == w->events.size()) {
            Event e;
            if (hipEventCreate(&e.a.h) != hipSuccess || hipEventCreate(&e.b.h) != hipSuccess) {
                on = false;
                return;
            }
            w->events.push_back(std::move(e));
        }
        idx = w->ev_used++;
        w->events[idx].cls = cls;
        (void)hipEventRecord(w->events[idx].a, s);
    }
    ~ProfScope()
    {
        if (on) (void)hipEventRecord(w->events[idx].b, s);
    }
};

// First pass with a sampled threshold.  Instead of bootstrapping on the first few thousand rows and
// growing the chunks geometrically (3-4 launches + selects per search), `count` evenly spaced rows of
// the first `span` positions are scored, their m-th best entry becomes the admission threshold and
// the whole span is then walked ONCE.  The threshold is only a filter: every row below it is collected,
// so a list that ends with >= keep entries holds exactly the span's best `keep`.
//   too tight:  fewer than `keep` rows pass iff >= m sampled rows are among the span's best keep-1;
//               that count is ~Poisson(lambda = keep*count/span), and m = lambda + 5 sqrt(lambda) + 4
//               puts the tail below 1e-6 (m = 10 for k = 100, 14 for the 256 MFMA candidates at 1M rows, 27-41 for the
//               1024 candidates the fp16 route keeps beyond 1024 dimensions);
//   too loose:  about m*span/count rows pass (1.2k-1.8k at 1M rows), relative spread 1/sqrt(m); the span
//               is capped so that mean + 5 sigma stays below the list capacity.
// Either miss is detected (flag bit 2 / bit 0) and the query is redone by the classic bootstrap
// schedule, so results never depend on the sample.  The stride makes the estimate independent of the
// row order (sorted or clustered corpora included).  Fewer admitted rows also matter for speed: each
// admission is a returning atomic on one hot counter, ~12 ns apiece in the 1-query scan.
static SamplePlan sample_plan_for(int64_t n, int keep, uint32_t cap, uint32_t count)
{
    SamplePlan p;
    int m = 8;
    int64_t span = 0;
    for (int it = 0; it < 8; it++) {
        const double loose = (double)m * (1.0 + 5.0 / std::sqrt((double)m)); // mean + 5 sigma, in units of span/count
        const double span_max = (double)(cap - (uint32_t)keep) * (double)count / loose;
        span = span_max >= (double)n ? n : (int64_t)span_max;
        const double lambda = (double)keep * (double)count / (double)span;
        const int need = (int)std::ceil(lambda + 5.0 * std::sqrt(lambda) + 4.0);
        if (need <= m) break;
        m = need;
        if (m > 64) return p; // (sample_tau_kernel: m pops of a minimum, m <= 64)
    }
    if (span < 8 * (int64_t)count || !sample_tau_supported(count, m)) return p;
    p.on = true;
    p.span = span;
    p.count = count;
    p.m = m;
    return p;
}
static SamplePlan sample_plan(int64_t n, int keep, uint32_t cap, uint32_t count_max = 8192u)
{
    // (round 4: sampled thresholds from 16,384 rows -- was 65,536: below it the classic schedule ran three corpus launches and
    // three selects where the sampled one runs a sample, one pass and the finish: 40k x 768 at 64 queries 0.19 -> 0.10 ms)
    static const int64_t sample_min_rows = lb_tunable("LB_SAMPLE_MIN_ROWS", 16384);
    if (!g_sample_tau.load() || n < sample_min_rows || (uint32_t)keep >= cap) return SamplePlan{};
    // the largest sample whose threshold rank stays within the kernel's reach and whose span covers the view: a small view
    // (a selective filter) or a long candidate list (large k) takes a smaller sample -- a sample that is a large share of
    // the rows would need its several-hundredth smallest entry
    SamplePlan best;
    for (uint32_t count = std::min<uint32_t>(cap, count_max); count >= 1024u; count >>= 1) {
        const SamplePlan p = sample_plan_for(n, keep, cap, count);
        if (!p.on) continue;
        if (!best.on || p.span > best.span) best = p;
        if (p.span >= n) break;
    }
    return best;
}

// Exact scan of all rows for the query slots sel[0..nsel) (indices into d_q rows).
// mode 0: sampled first pass, 1: classic (bootstrap / growing chunks), 2: chunks that cannot overflow.
bool run_scan_path(lb_gpu_index *h, Workspace *w, hipStream_t s, const float *d_q, const int *d_sel,
                   int nsel, int k, int mode, float *d_dist, int64_t *d_lab, bool prof)
{
    const int metric = h->metric, order = h->order.load();
    const IndexRowView rv = row_view(h, w);
    const int64_t n = rv.n;
    const uint8_t *mask = rv.mask;
    const int kkeep = std::max(k, 1);
    const bool safe = mode == 2;
    // (the latency path samples half as many rows: the sample launches are on its critical path, and the
    // extra admissions -- ~2k instead of ~1.2k at 1M rows -- are spread over the striped counters)
    static const uint32_t scan_count = (uint32_t)lb_tunable("LB_SCAN_SAMPLE", 4096);
    const SamplePlan sp = mode == 0 ? sample_plan(n, kkeep, w->cap, scan_count) : SamplePlan{};
    if (!sp.on) launch_init_cand(w->cs, d_sel, nsel, s);
    for (int g0 = 0; g0 < nsel; g0 += kScanMaxQ) {
        ctx_check(w->ctx);
        const int gn = std::min(kScanMaxQ, nsel - g0);
        const int *use_sel = d_sel + g0; // d_sel is always an explicit slot list here
        int64_t pos = 0;
        int step = 0;
        bool emitted = false;
        const EmitArgs em{k, h->has_ids ? h->d_ids.get() : nullptr, d_dist, d_lab, w->h_flags.get()};
        if (sp.on) {
            {   // sample scores (clear the flags; exact query norms ride along), threshold
                ProfScope p(w, s, prof, 1);
                if (h->i8_rows)
                    launch_sample_scores_i8(metric, h->rows_i8(), h->dim, sp.span, sp.count, rv.rowmap, mask, d_q, use_sel, gn, w->cs, s);
                else
                    with_rows(h, [&](auto X) {
                        launch_sample_scores(metric, order, X, h->dim, sp.span, sp.count, rv.rowmap, mask, d_q, use_sel, gn, w->cs,
                                             w->d_qna.get(), s);
                    });
                launch_sample_tau(w->cs, use_sel, gn, sp.count, sp.m, /*zero_stripes=*/true, s);
            }
            {   // one pass over the span
                ProfScope p(w, s, prof, 3);
                if (h->i8_rows)
                    launch_scan_i8(metric, h->rows_i8(), 0, sp.span, h->dim, d_q, use_sel, gn, h->norm2_i8(), mask, rv.rowmap, w->cs,
                                   /*boot=*/false, s, /*striped=*/true);
                else
                    with_rows(h, [&](auto X) {
                        launch_scan(metric, order, false, X, 0, sp.span, h->dim, d_q, use_sel, gn, w->d_qna.get(), mask, rv.rowmap, w->cs,
                                    /*boot=*/false, nullptr, 0, s, /*striped=*/true);
                    });
            }
            {
                ProfScope p(w, s, prof, 1);
                launch_select(w->cs, use_sel, gn, kkeep, 0u, s, (uint32_t)kkeep, sp.span >= n ? &em : nullptr,
                              /*striped=*/true);
            }
            pos = sp.span;
            step = 1;
            emitted = sp.span >= n;
        } else if (metric == LB_METRIC_COSINE) {
            ProfScope p(w, s, prof, 3);
            launch_query_norms(order, d_q, use_sel, gn, h->dim, w->d_qna.get(), s);
        }
        while (pos < n) {
            ctx_check(w->ctx);
            const int64_t end = chunk_end_host(step, pos, n, kkeep, w->cap, safe, /*big_boot=*/true);
            const bool boot = step == 0;
            {
                ProfScope p(w, s, prof, 3);
                if (h->i8_rows)
                    launch_scan_i8(metric, h->rows_i8(), pos, end, h->dim, d_q, use_sel, gn, h->norm2_i8(), mask, rv.rowmap, w->cs,
                                   boot, s, /*striped=*/false);
                else
                    with_rows(h, [&](auto X) {
                        launch_scan(metric, order, false, X, pos, end, h->dim, d_q, use_sel, gn, w->d_qna.get(), mask, rv.rowmap, w->cs,
                                    boot, nullptr, 0, s);
                    });
            }
            {
                ProfScope p(w, s, prof, 1);
                launch_select(w->cs, use_sel, gn, kkeep, boot ? (uint32_t)(end - pos) : 0u, s, 0u,
                              end >= n ? &em : nullptr);
            }
            emitted = end >= n;
            pos = end;
            step++;
        }
        if (!emitted) // (only an empty corpus view gets here)
            launch_emit_lists(w->cs, use_sel, gn, k, h->has_ids ? h->d_ids.get() : nullptr, d_dist, d_lab, w->h_flags.get(), s);
    }
    return sp.on;
}

// download flags for slots [0,nq) and return those with any of `bits` set
// (on_host: the last kernel already wrote the subset's flags into the pinned h_flags)
int collect_flagged(Workspace *w, hipStream_t s, int nq, uint32_t bits, const int *h_subset,
                    int nsubset, std::vector<int> &out, bool on_host = false)
{
    if (!on_host)
        LB_HIP(hipMemcpyAsync(w->h_flags.get(), w->cs.flags, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    out.clear();
    if (h_subset) {
        for (int i = 0; i < nsubset; i++)
            if (w->h_flags.get()[h_subset[i]] & bits) out.push_back(h_subset[i]);
    } else {
        for (int i = 0; i < nq; i++)
            if (w->h_flags.get()[i] & bits) out.push_back(i);
    }
    return (int)out.size();
}

void upload_sel(Workspace *w, hipStream_t s, const std::vector<int> &sel)
{
    std::memcpy(w->h_qsel.get(), sel.data(), sel.size() * sizeof(int));
    LB_HIP(hipMemcpyAsync(w->d_qsel.get(), w->h_qsel.get(), sel.size() * sizeof(int), hipMemcpyHostToDevice, s));
}

// exact scan of the query slots in `sel` of a batch of nq, or (sel null) of every query of the batch
void scan_with_retry(lb_gpu_index *h, Workspace *w, hipStream_t s, const float *d_q, int nq,
                     const std::vector<int> *sel, int k, float *d_dist, int64_t *d_lab, bool prof)
{
    const int nsel = sel ? (int)sel->size() : nq;
    if (nsel == 0) return;
    bool identity = true; // slots 0, 1, ...: the prefilled list saves an upload on the latency path
    for (int i = 0; sel && i < nsel && identity; i++) identity = (*sel)[(size_t)i] == i;
    if (!identity) upload_sel(w, s, *sel);
    const bool sampled = run_scan_path(h, w, s, d_q, identity ? w->d_iota.get() : w->d_qsel.get(), nsel, k, 0, d_dist, d_lab, prof);
    std::vector<int> redo, over;
    if (collect_flagged(w, s, nq, 1u | 4u, sel ? sel->data() : nullptr, nsel, redo, true) > 0) {
        // the sampled threshold missed (or a list overflowed): classic schedule, then overflow-proof chunks
        if (sampled) {
            upload_sel(w, s, redo);
            run_scan_path(h, w, s, d_q, w->d_qsel.get(), (int)redo.size(), k, 1, d_dist, d_lab, prof);
        }
        if (!sampled || collect_flagged(w, s, nq, 1u, redo.data(), (int)redo.size(), over, true) > 0) {
            if (!sampled) over = redo;
            upload_sel(w, s, over);
            run_scan_path(h, w, s, d_q, w->d_qsel.get(), (int)over.size(), k, 2, d_dist, d_lab, prof);
            LB_HIP(hipStreamSynchronize(s));
        }
    }
}

// ---- which kernel generates the candidates of a batch ----------------------------------------------------------
// Every route is exact (re-rank + containment proof, else the exact scan redoes the query), so this is a cost choice.
//   NARROW32 / NARROW64  256 x 32 or 128 x 64 tile, operands split to bf16 in registers: one HBM-bound corpus pass per
//                        32 / 64 queries (kernels_gemm_narrow.hip)
//   TALL2                256 x 256 tile on the split contraction (kernels_gemm_tall2.hip): corpus image (split 1) or f32
//                        corpus split in registers (split 2)
//   TALL16 / NARROW16    ONE fp16 product per element (kernels_gemm_tall16.hip): 256 x 256 tiles, or one 64- / 128-query
//                        tile over the index's fp16 image (persistent workgroups, LDS-DMA ring)
//   WIDE                 128 x 128 tile (kernels_gemm.hip): f32 MFMA (split 0), the strict mode's route beyond 384 queries
// Candidate modes (lb_gpu_index_set_candidate_mode):
//   LB_CAND_AUTO (default)    the cheapest route by the cost model below -- with the fp16 image that is the single-product
//                             route at every batch size, the split contraction where the data's range rules fp16 keys out
//   LB_CAND_F32_MFMA          as AUTO up to 384 queries, the f32-MFMA 128 x 128 tile beyond (rounds 1-2 default)
//   LB_CAND_SPLIT_BF16        corpus image for everything beyond the narrow tiles
//   LB_CAND_SPLIT_BF16_INREG  in-register split for everything beyond the narrow tiles
// Cost model: a pass over `n` positions of dimension D costs  n * (alpha * D + beta) [+ gamma]  per query tile, with
// the constants measured per kernel on MI355X over D in {128 .. 1536} x n in {100k .. 10M} (tools/route_grid.py; the
// GPU test test_route_choice_is_near_the_best_forced_route checks the choice against every forced route).
enum RouteKind { ROUTE_NARROW32 = 1, ROUTE_NARROW64 = 2, /* 3: the 256 x 128 split tile of rounds 2-3, removed */ ROUTE_WIDE = 4, ROUTE_TALL2 = 5, ROUTE_TALL16 = 6,
                 ROUTE_NARROW16 = 7 /* the fp16 route's 64- / 128-query tile over the fp16 copy: same pipeline as TALL16, reported apart */ };
struct Route {
    int kind = ROUTE_WIDE;
    int split = 0;
    double cost_ms = 0;
};
// One pass of a route's kernel over n positions of dimension D with `tiles` query tiles costs
//     ms = max(tiles * 1e-6 * n * (alpha * D + beta),  1e-6 * n * D * hbm)  +  1e-6 * n * D * first
// alpha: the contraction (per position, dimension and query tile); beta: the per-position work that does not scale with
// D (epilogue: key, admission test, side inputs); hbm: the corpus stream under that kernel (4 bytes per element at the
// rate the kernel's staging reaches); first: what the first query tile of a multi-tile pass waits for the corpus.
// Fitted to tools/route_grid.py on MI355X (D in {128, 384, 768, 1536} x n in {100k, 1M, 4M}), see LABNOTES.md 3.2.
struct RouteCost {
    double alpha, beta, hbm, first;
    double fixed = 0; // ms per search whatever the corpus: launches, thresholds, select, re-rank (fp16: + the query image, twice the
                      // candidates; the one-tile form over the fp16 copy: its re-rank is counted per query)
};
// (narrow tiles: one launch, the corpus tile is read from HBM once and re-used from L2 by the other query tiles)
constexpr RouteCost kCostNarrow32{0.000323, 0.0247, 0.000640, 0.000300, 0.09};   // per 32-query tile: 1.09 ms at 4M x 768, 0.27 at 4M x 128
constexpr RouteCost kCostNarrow64{0.000527, 0.0225, 0.000640, 0.000200, 0.09};   // per 64-query tile: 1.71 ms at 4M x 768, 0.36 at 4M x 128
constexpr RouteCost kCostTall2Inreg{0.001260, 0.1300, 0.000640, 0.000250, 0.09}; // per 256-query tile: 3.9 ms at 4M x 768, 1.16 at 4M x 128
constexpr RouteCost kCostTall2Image{0.001150, 0.1300, 0.000640, 0.000220, 0.09};
constexpr RouteCost kCostWideF32{0.001940, 0.0600, 0.000640, 0.0, 0.09};
constexpr RouteCost kCostTall16{0.000540, 0.0800, 0.000660, 0.000140, 0.19}; // per 256-query tile, one fp16 product, persistent form: 0.49 ms per
                                                                             // tile at 1M x 768, a single tile streams the corpus at 6 TB/s
constexpr RouteCost kCostTall16Img{0.000460, 0.0500, 0.000330, 0.000040, 0.11}; // the same from the corpus's fp16 image: 0.40 ms per tile at
                                                                                // 1M x 768, never bound by the stream (1.5 GB)
constexpr RouteCost kCostNarrow16{0.000100, 0.0300, 0.000340, 0.000030, 0.06};  // up to 64 queries over the fp16 copy: its HBM stream (6 TB/s)
inline double route_ms(const RouteCost &c, int64_t n, int D, int tiles)
{
    const double nd = 1e-6 * (double)n;
    const double compute = (double)tiles * nd * (c.alpha * (double)D + c.beta);
    const double stream = nd * (double)D * c.hbm;
    return (compute > stream ? compute : stream) + nd * (double)D * c.first + c.fixed;
}
// the one-tile fp16 route over the image for nq <= 128 queries: its stream + what it pays per query beside it -- twice (beyond 1024
// dimensions four times) the candidates to select and re-rank
// (round 4: 0.0016 -> 0.0008 beyond 1024 dimensions -- the finish launch re-ranks ~270 rows per query where select + re-rank scored
// 1024; with 0.0016 a row list of 125k x 1536 went to the 64-query split tile at exactly 64 and 128 queries: 0.30 / 0.40 ms where
// the image serves them in 0.24 / 0.31)
inline double narrow16_ms(int64_t n, int D, int nq) { return route_ms(kCostNarrow16, n, D, 1) + (D > 1024 ? 0.0008 : 0.0003) * nq; }

// Candidates the fp16 single-product route keeps per query for a list of kc (mult > 0: that many times kc instead).  Its keys are
// good to ~1.1e-3 of |q||x|, and the containment proof needs the gap between the k-th and the LAST kept candidate to exceed about
// 2.5x that -- on the benchmark data the gap to the 256th is 0.0019-0.0028 (most queries would fail), to the 512th 0.0039-0.0045.
// (Uniform random data is the hard case: its distances concentrate like 1/sqrt(D), so the gap shrinks with the dimension while
// the bound does not -- beyond 1024 dimensions four times as many candidates are kept.)
// (since the finish launch prunes in key space, kc only sizes the admission threshold: the list must hold the rows within the
// error bound of the k-th key -- 2-4 k of them with fp16 keys -- not a fixed number of rows to re-rank; capped so that a sampled
// threshold of that depth still exists)
inline int f16_kc(int kc, int D, uint32_t cap, int mult = 0)
{
    return std::min(std::min(kc * (mult > 0 ? mult : (D > 1024 ? 4 : 2)), std::max(1024, 2 * kc)), (int)(cap / 4));
}

// f32_rows false (an fp16 index): only the routes over the fp16 image are offered -- every other one stages f32 rows; with none
// on offer the result has kind 0 (the exact scan)
static Route choose_route(int nq, int64_t n, int D, int cmode, bool narrow_ok, bool have_image, bool f16_ok, bool have_f16_image = false,
                          bool f32_rows = true)
{
    static const int narrow_max = lb_tunable("LB_NARROW_MAXQ", 384);
    const int tiles32 = (nq + 31) / 32, tiles64 = (nq + 63) / 64, tiles128 = (nq + 127) / 128, tiles256 = (nq + 255) / 256;
    // (tall tiles only with enough of them to fill the chip a few times over: 512 workgroups run at once, and at 125k
    // visible rows x 256 queries the 978 tall tiles came out 5 % behind the 3908 smaller ones)
    const bool tall2_fills = (n / 256) * tiles256 >= 1024; // (one workgroup per CU: 256 run at once)
    Route cand[8];
    int nc = 0;
    auto add = [&](int kind, int split, double ms) { cand[nc].kind = kind; cand[nc].split = split; cand[nc].cost_ms = ms; nc++; };
    const bool image = cmode == LB_CAND_SPLIT_BF16 && have_image;
    if (!f32_rows) narrow_ok = false;
    if (narrow_ok && !image && (cmode == LB_CAND_AUTO || nq <= narrow_max)) {
        if (nq <= 32 || tiles32 <= 10) add(ROUTE_NARROW32, 2, route_ms(kCostNarrow32, n, D, tiles32));
        if (nq > 32) add(ROUTE_NARROW64, 2, route_ms(kCostNarrow64, n, D, tiles64));
    }
    // (round 4: the 256 x 128 tile -- ROUTE_TALL, kernels_gemm_tall.hip -- is gone: within 2-5 % of the 64-query narrow tile and of
    // this one wherever it was picked, profiles/r03_route_grid.txt, and never picked once the fp16 route is on offer)
    if (narrow_ok) {
        if (image) {
            add(ROUTE_TALL2, 1, route_ms(kCostTall2Image, n, D, tiles256));
        } else if (cmode != LB_CAND_F32_MFMA || nq <= narrow_max) {
            const bool forced = cmode == LB_CAND_SPLIT_BF16_INREG;
            if (nq > 128 && (tall2_fills || forced)) add(ROUTE_TALL2, 2, route_ms(kCostTall2Inreg, n, D, tiles256));
        }
    }
    // one fp16 product instead of three bf16 ones (split code 3): AUTO and the explicit LB_CAND_F16, while the corpus norms
    // allow it (f16_ok) and there are enough tiles to fill the chip
    // (a filtered view of a corpus that has its fp16 image: from the size a sampled threshold exists for, the cost model
    // decides -- round 3's gate of 128 Mi elements kept 100k x 768 views on the 64-query split tile: 0.21 / 0.30 / 0.50 ms at
    // 128 / 256 / 512 queries where the image serves them in 0.16 / 0.20 / 0.28)
    static const int64_t f16_view_min = lb_tunable("LB_F16_VIEW_MIN", 16384);
    // (over the fp16 copy the route needs neither dim % 32 == 0 nor aligned queries: both images are zero-padded planes)
    if ((narrow_ok || have_f16_image) && f16_ok && !image && (nq > 32 || have_f16_image) &&
        (cmode == LB_CAND_F16 || (cmode == LB_CAND_AUTO && (n >= 262144 || (have_f16_image && n >= f16_view_min)))))
    { // (below: launch overheads decide, and the narrow tiles win; a filtered view of a large corpus counts by its elements)
        if (have_f16_image && nq <= 128) add(ROUTE_NARROW16, 3, narrow16_ms(n, D, nq)); // (one query tile: the 64- / 128-query
                                                                                       // form of the persistent kernel)
        else add(ROUTE_TALL16, 3, route_ms(have_f16_image ? kCostTall16Img : kCostTall16, n, D, tiles256));
    }
    if (!f32_rows && nc == 0) return Route{0, 0, 0.0};
    if (f32_rows && (cmode == LB_CAND_F32_MFMA || cmode == LB_CAND_AUTO || nc == 0)) add(ROUTE_WIDE, 0, route_ms(kCostWideF32, n, D, tiles128));
#ifdef LB_DIAG
    { // A/B (tools/route_grid.py): force a route when it is available for this batch (read per call: the tool flips it)
        if (getenv("LB_TRACE_ROUTE")) {
            fprintf(stderr, "[route] nq %d n %lld D %d cmode %d narrow_ok %d f16_ok %d image %d:", nq, (long long)n, D, cmode, (int)narrow_ok, (int)f16_ok, (int)have_f16_image);
            for (int i = 0; i < nc; i++) fprintf(stderr, " kind %d/%d %.3f ms", cand[i].kind, cand[i].split, cand[i].cost_ms);
            fprintf(stderr, "\n");
        }
        const char *e = getenv("LB_FORCE_ROUTE");
        const int force = e ? atoi(e) : 0;
        for (int i = 0; i < nc; i++)
            if (cand[i].kind == force) return cand[i];
    }
#endif
    if (cmode == LB_CAND_F32_MFMA && nq > narrow_max) return cand[nc - 1]; // strict mode: the f32 tile beyond the narrow range
    if (cmode == LB_CAND_F16)
        for (int i = 0; i < nc; i++)
            if (cand[i].kind == ROUTE_TALL16 || cand[i].kind == ROUTE_NARROW16) return cand[i];
    if (nq <= 32 && nc > 0 && cand[0].kind == ROUTE_NARROW32) {
        // one pass of the 32-query tile (sample and thresholds inside the launch): 0.09 ms + 0.47 ms per 1M x 768 whatever the
        // model above says about tile counts -- nothing is cheaper but the stream of the fp16 copy
        cand[0].cost_ms = 0.09 + 1e-6 * (double)n * (0.014 + 0.000612 * (double)D);
        for (int i = 1; i < nc; i++)
            if (cand[i].kind == ROUTE_NARROW16 && cand[i].cost_ms < cand[0].cost_ms) return cand[i];
        return cand[0];
    }
    int best = 0;
    for (int i = 1; i < nc; i++)
        if (cand[i].cost_ms < cand[best].cost_ms) best = i;
    return cand[best];
}

// what lb_gpu_index_last_route (and, in the diagnostic build, lb_debug_last_route) reports of the most recent batched search
void note_route(lb_gpu_index *h, int code)
{
    h->last_route.store(code, std::memory_order_relaxed);
#ifdef LB_DIAG
    g_last_route.store(code);
#endif
}

// An int8 index's batch (kernels_i8.hip).  Every kernel there computes the exact reference value of each (row, query) pair, so
// the candidate entries are the results themselves: no candidate keys, no finish, no containment bound.
//   route 80  the exact scan (run_scan_path): 8 queries a corpus pass, v_dot4c_i32_i8;
//   route 81  the i8 MFMA pass: 128 queries a corpus pass.  Its sampled threshold comes from the same kernel over the sampled
//             positions; the one select behind the pass emits.  A query whose list overflowed or ended short (flags 1 / 4) is
//             redone by the scan.  Needs D % 16 == 0 (dot: D <= 1024), 16-B aligned query rows and a sampled span that covers
//             the row view; batches from LB_I8_MFMA_MINQ queries.
// d_q: the batch widened to f32 (the scan's input), d_q8: the same queries as int8 (the MFMA pass's).
constexpr int kRouteI8Scan = 80, kRouteI8Mfma = 81;
int search_batch_i8(lb_gpu_index *h, Workspace *w, hipStream_t s, int nq, const float *d_q, const int8_t *d_q8, int k, float *d_dist,
                    int64_t *d_lab, bool prof)
{
    static const int mfma_minq = lb_tunable("LB_I8_MFMA_MINQ", 16);
    const IndexRowView rv = row_view(h, w);
    const int kkeep = std::max(k, 1);
    SamplePlan sp;
    if (nq >= mfma_minq && mfma_i8_supported(h->metric, h->dim, h->d_X, d_q8)) sp = sample_plan(rv.n, kkeep, w->cap);
    if (!sp.on || sp.span < rv.n) {
        note_route(h, kRouteI8Scan);
        scan_with_retry(h, w, s, d_q, nq, nullptr, k, d_dist, d_lab, prof);
        return LB_OK;
    }
    note_route(h, kRouteI8Mfma);
    int32_t *qn = reinterpret_cast<int32_t *>(w->d_qna.get()); // (nq_cap words: the exact int32 |q|^2 here)
    {
        ProfScope p(w, s, prof, 1);
        LB_HIP(hipMemsetAsync(w->cs.flags, 0, (size_t)nq * sizeof(uint32_t), s));
        launch_query_norms_i8(d_q8, nq, h->dim, qn, s);
        launch_mfma_i8(h->metric, h->rows_i8(), sp.count, h->dim, d_q8, nq, qn, h->norm2_i8(), rv.mask, rv.rowmap, w->cs,
                       /*sample=*/true, sp.span, s);
        launch_sample_tau(w->cs, nullptr, nq, sp.count, sp.m, /*zero_stripes=*/false, s);
    }
    {
        ProfScope p(w, s, prof, 3);
        launch_mfma_i8(h->metric, h->rows_i8(), rv.n, h->dim, d_q8, nq, qn, h->norm2_i8(), rv.mask, rv.rowmap, w->cs,
                       /*sample=*/false, rv.n, s);
    }
    {
        ProfScope p(w, s, prof, 1);
        const EmitArgs em{k, h->has_ids ? h->d_ids.get() : nullptr, d_dist, d_lab, w->h_flags.get()};
        launch_select(w->cs, nullptr, nq, kkeep, 0u, s, (uint32_t)kkeep, &em);
    }
    std::vector<int> redo;
    if (collect_flagged(w, s, nq, 1u | 4u, nullptr, 0, redo, true) > 0)
        scan_with_retry(h, w, s, d_q, nq, &redo, k, d_dist, d_lab, prof);
    return LB_OK;
}

// Rounding-error bound of a route's candidate inner products, per unit of ||q|| ||x|| (the finish launch's containment proof):
// a k-ordered f32 fma chain of length D, or (split contraction) 3D/16 MFMA accumulations + <=16-term block sums plus the dropped
// lo*lo / residual terms
// ... or (split 3) one fp16 product: 2^-11 per operand, the subnormal term under the route's norm conditions, and the
// f32 accumulation of D products (kernels_gemm_tall16.hip)
// ... with the index's fp16 image the operands' share is MEASURED instead: |q.x - q~.x~| <= |q||x - x~| + |q - q~||x~|, the
// residual norms taken when the image was written (rho_x = max over rows of |x - x~| / |x|, sync_f16_image) and when the
// query image is (rho_q per query, query_prep_body) -- a third to a half of the worst case for data that fills the
// mantissa, subnormal effects included:  gamma(q) = 1.05 (rho_x + A (1 + rho_x) + 2^-21) + 1.05 (1 + rho_x)(1 + A) rho_q,
// A = (D + 8) 2^-24 the f32 accumulation of D exact products
struct KeyBound {
    bool measured; // gamma(q) = gamma + qrho_k * rho_q
    float gamma, qrho_k;
    // dot product on the persistent fp16 kernels: LOWER-BOUND keys -(q.x)~ / G - |x|, G = (gamma_a + gamma_o) |q| = gsum |q| (a few
    // very long rows then sort to the front of the lists and are scored exactly instead of widening every row's error bound)
    float gsum, rho_gain; // (measured, dot: G(q) = (gsum + qrho_k rho_q) |q|, folded into qnrm)
};
KeyBound key_bound(const lb_gpu_index *h, int split, bool have_xh)
{
    const float u24 = 5.9604645e-8f;
    KeyBound b;
    b.measured = split == 3 && have_xh && (h->xh_rho > 0.f || h->xh_exact) &&
                 h->xh_rho < 4.0e-4f; // (else the worst case is the better bound)
    const float accA = (float)(h->dim + 8) * u24;
    b.qrho_k = b.measured ? 1.05f * (1.0f + h->xh_rho) * (1.0f + accA) : 0.f;
    b.gamma = split == 0     ? 1.05f * (float)(h->dim + 8) * u24
              : b.measured   ? 1.05f * (h->xh_rho + accA * (1.0f + h->xh_rho) + 4.7683716e-7f)
              : split == 3   ? 1.05f * (9.765625e-4f + 4.7683716e-7f + (float)(h->dim + 8) * u24 +
                                        2.9802322e-8f * std::sqrt((float)h->dim) * 65.0f)
                             : 1.05f * ((float)(3 * h->dim / 16 + 24) * u24 + 3.0f * 3.8146973e-6f);
    b.gsum = b.gamma + 1.05f * (float)(h->dim + 8) * u24;
    b.rho_gain = (b.measured && b.gsum > 0.f) ? b.qrho_k / b.gsum : 0.f;
    return b;
}

// the rows behind the plan's sampled positions: the index's shared map (built by the first search after a change), or when that
// holds another plan, the workspace's own -- always the workspace's own under a call's view (Workspace::call_view): the shared
// map is the handle's view's, neither read nor published by a call that brought its own bitmap
const uint32_t *sample_map(lb_gpu_index *h, Workspace *w, hipStream_t s, const IndexRowView &rv, const SamplePlan &sp)
{
    if (!w->call_view) {
        std::lock_guard<std::mutex> g(h->smap_mu);
        if (!h->smap_valid) {
            h->d_smap.ensure(sp.count);
            launch_sample_map(rv.rowmap, sp.span, sp.count, h->d_smap.get(), s);
            LB_HIP(hipStreamSynchronize(s));
            h->smap_span = sp.span;
            h->smap_count = sp.count;
            h->smap_valid = true;
        }
        if (h->smap_span == sp.span && h->smap_count == sp.count) return h->d_smap.get();
    }
    launch_sample_map(rv.rowmap, sp.span, sp.count, w->d_smap.get(), s);
    return w->d_smap.get();
}

// How a batched search scores the sample of its thresholds (one way per search; NONE: no sampled threshold):
//   FUSED    up to 64 queries on the narrow split tiles: the sample and its thresholds ride INSIDE the candidate launch
//            (FUSED in kernels_gemm_narrow.hip: 19-34 us of sample + 13 us of threshold kernel off the critical path)
//   GRANULE  over the fp16 copy: through the persistent kernel itself, 512 granules of 16 consecutive rows, evenly spaced over
//            the span (whole KiB of the K-blocked image; every workgroup takes a share of them)
//   LIGHT    up to 8 queries: the wave-per-row kernel (candidate keys; 22-28 us against 44 us for 8192 rows through the
//            32-workgroup MFMA launch, and 5 us quicker than the granules: every load of a row in flight at once)
//   MAPPED   the sampled rows' map (sample_map), scored by the candidate launch itself
enum SampleKind { SAMPLE_NONE, SAMPLE_FUSED, SAMPLE_GRANULE, SAMPLE_LIGHT, SAMPLE_MAPPED };
// narrow / tall16: the route's tiles (the narrow split tiles / the fp16 kernels); entries_pos: the pass's entries carry positions of
// the row list (a row list on the persistent fp16 kernels); dot_lb: dot product's lower-bound keys (those kernels too)
SampleKind sample_kind(const SamplePlan &sp, bool narrow, bool tall16, int nq, int64_t n, bool rowmap, bool entries_pos, bool have_xh,
                       bool dot_lb)
{
    static const int fused_max = lb_tunable("LB_FUSED_SAMPLE_MAXQ", 32); // (33-64 queries, the 64-query tile: measured level)
    static const int light_max = lb_tunable("LB_LIGHT_SAMPLE_MAXQ", 8); // (also over a row list: at 32 queries the wave-per-row
                                                                        // kernel took 105 us against the granule sample's 40)
    if (!sp.on) return SAMPLE_NONE;
    // (fused from 131,072 rows: the fused launch has a floor of ~115 us whatever the corpus -- 70k x 768 at 8 queries 0.156 ms fused,
    // 0.124 with the sample and the thresholds as launches of their own, level at 150k-300k, 20 us ahead at 1M -- and on the
    // 16k-64k-row corpora that take a sampled threshold since round 4 its waits gave up: 17k rows at 16 queries, 40k at 32,
    // the batch redone exactly in 1 ms)
    // (and thresholds of rank up to 32: with k = 300 -- 1024 candidates, m = 48 -- the threshold workgroups outlast the waits of
    // the corpus workgroups: 200k x 768 at 32 queries gave up on every search, 1.5 ms)
    if (narrow && nq <= fused_max && nq <= 64 && n >= 131072 && sp.m <= 32) return SAMPLE_FUSED;
    // (dot product's lower-bound keys: the sample must come out of the same kernel; centred L2 keys the wave-per-row kernel
    // computes too, from the f32 rows about the same centre)
    if (tall16 && sp.count % 16 == 0 && (!rowmap || entries_pos) &&
        ((have_xh && nq > light_max) || dot_lb))
        return SAMPLE_GRANULE;
    // (not in front of the split tiles: up to 32 queries they always ran fused, and the wave-per-row sample was never paired
    // with them -- L2, k = 300, 8 queries over 50k rows: every query flagged and scanned)
    return nq <= light_max && !narrow ? SAMPLE_LIGHT : SAMPLE_MAPPED;
}

// One attempt of a batched search on `route`, keeping kc candidates per query: the sampled threshold, the candidate pass over the
// view and the finish (key-space pruning + exact re-rank + containment proof).  Returns how many queries it left unproven, their
// slots in `bad` -- or, when a wait inside the fused launch gave up (gave_up), every query of the batch (`bad` is then not filled).
int run_batch(lb_gpu_index *h, Workspace *w, hipStream_t s, int nq, const float *d_q, int k, float *d_dist, int64_t *d_lab, bool prof,
              const Route &route, int kc, bool narrow_ok, bool have_xh, std::vector<int> &bad, bool &gave_up)
{
    const int metric = h->metric, order = h->order.load();
    const IndexRowView rv = row_view(h, w);
    const int64_t n = rv.n;
    const uint8_t *mask = rv.mask;
    const SamplePlan sp = sample_plan(n, kc, w->cap);
    // candidate contraction: exact f32 MFMA, 3 x bf16 MFMA on split operands, or one fp16 product (choose_route)
    const bool use_narrow = route.kind == ROUTE_NARROW32 || route.kind == ROUTE_NARROW64;
    const bool tile64 = route.kind == ROUTE_NARROW64;
    const bool use_tall2 = route.kind == ROUTE_TALL2;
    const bool use_tall16 = route.kind == ROUTE_TALL16 || route.kind == ROUTE_NARROW16; // (the launcher takes the 64-query tile by itself)
    const int wsplit = use_narrow ? 0 : route.split; // of the operands handed to the kernel: 0 f32, 1 images, 2 f32 split in registers
    const bool centred = have_xh && h->xh_centred;   // L2 image about a centre (sync_f16_image)
    // the keys of this search are taken about the image's centre: sample, pass and finish read the centred norms and the centre
    const bool ckeys = centred && use_tall16;
    const float *knorm2 = ckeys ? h->d_norm2c.get() : h->d_norm2.get(), *kcenter = ckeys ? h->d_center.get() : nullptr;
    const KeyBound kb = key_bound(h, route.split, have_xh);
    const float *gx = h->d_X, *gq = d_q;
    if (!use_narrow && (route.split == 1 || route.split == 2)) { // the tall / wide split kernels take the batch as an image
        w->d_qs.ensure((size_t)nq * h->dim); // (hi / lo bf16: the bytes of the f32 rows)
        launch_split_bf16(d_q, w->d_qs.get(), nq, h->dim, s);
        if (route.split == 1) {
            gx = h->d_Xs.get();
            gq = w->d_qs.get();
        }
    }
    float *d_qinv = nullptr, *d_qnrm = nullptr, *d_qrho = nullptr;
    // dot product on the persistent fp16 kernels: LOWER-BOUND keys (KeyBound::gsum)
    const bool dot_lb = metric == LB_METRIC_DOT && use_tall16 &&
                        tall16_runs_persistent(h->dim, nq, have_xh, rv.rowmap != nullptr, mask != nullptr);
    const bool own_keys = centred || dot_lb; // keys only the persistent kernels produce: sample and boot chunks must come from them
    static const int riders_max = lb_tunable("LB_NORM_RIDERS_MAXQ", 384);
    const bool prep_riders = sp.on && nq <= riders_max; // (cosine: the exact query norms come out of the threshold launch)
    const bool norm_riders = prep_riders && metric == LB_METRIC_COSINE;
    if (use_tall16) { // fp16 image of the batch (scaled per query) + the inverse scales
        const size_t img = (((size_t)nq * (size_t)((h->dim + 31) & ~31) * 2) + 255) & ~(size_t)255;
        w->d_qh.ensure(img + 3 * (size_t)nq * sizeof(float));
        d_qinv = reinterpret_cast<float *>(w->d_qh.get() + img);
        d_qnrm = d_qinv + nq;
        d_qrho = kb.measured ? d_qnrm + nq : nullptr;
    }
    // a search over a row list on the persistent fp16 kernels: its candidate entries carry positions of the list
    const bool entries_pos = use_tall16 && rv.rowmap != nullptr &&
                             tall16_entries_are_positions(h->dim, nq, have_xh, true, mask != nullptr);
    const SampleKind sample = sample_kind(sp, use_narrow, use_tall16, nq, n, rv.rowmap != nullptr, entries_pos, have_xh, dot_lb);
    // Up to 128 queries on the one-tile kernel over the image, one span: the candidate launch turns the sample into the
    // thresholds ITSELF (its first nq workgroups, on shorter row ranges; kernels_gemm_tall16.hip, TAUIN) -- no threshold launch
    // and no gap behind it in front of the pass.
    const bool tauin = (sample == SAMPLE_LIGHT || sample == SAMPLE_GRANULE) && sp.span >= n && route.kind == ROUTE_NARROW16 &&
                       prep_riders &&
                       tall16_tin_ok(h->dim, nq, sp.span, have_xh, rv.rowmap != nullptr, mask != nullptr, norm_riders, sp.count, sp.m);
    Tall16Tin tin{};
    uint32_t tin_epoch = 0;
    if (tauin) {
        tin_epoch = w->next_epoch();
        tin.count = sp.count;
        tin.m = sp.m;
        tin.tag = tin_epoch;
        tin.fail_host = w->h_fail.get();
        tin.Q = d_q;
        tin.qna = norm_riders ? w->d_qna.get() : nullptr;
        tin.order = order;
#ifdef LB_DIAG
        tin.withhold = g_tin_withhold_next.exchange(0);
#endif
    }
    // (up to 8 queries: the query preparation rides in the sample launch -- one launch and one gap less in front of the pass)
    const bool prep_rides = use_tall16 && sample == SAMPLE_LIGHT && prep_riders;
    if (use_tall16 && !prep_rides)
        // one launch: the image, the scales, the exact query norms (cosine) and the reset of the candidate state
        // (the exact norm is a serial chain of D additions, 3.5 us at 768: up to 384 queries it rides in the threshold launch
        // instead, where nothing waits for it)
        launch_query_prep(d_q, nq, h->dim, w->d_qh.get(), d_qinv, (metric == LB_METRIC_COSINE && !prep_riders) ? w->d_qna.get() : nullptr, order,
                          w->cs, s, kcenter, dot_lb ? d_qnrm : nullptr, tauin, d_qrho, kb.rho_gain);
    // the last launch: key-space pruning + exact re-rank + proof in one (kernels_finish.hip); beta: how far beyond one error
    // bound the cut lies (the proof itself never depends on it)
    static const float finish_beta = 0.01f * (float)lb_tunable("LB_FINISH_BETA_PCT", 25);
    if (sample != SAMPLE_LIGHT && sample != SAMPLE_FUSED && !use_tall16) launch_init_cand(w->cs, nullptr, nq, s);
    if (metric == LB_METRIC_COSINE && !norm_riders && !use_tall16) launch_query_norms(order, d_q, nullptr, nq, h->dim, w->d_qna.get(), s); // (fp16 route: query_prep)
    // (fp16 route, several 256-query tiles: the sample goes through the fp16 kernel itself -- 32 row tiles x nq/256 workgroups
    // against nq/64 x 64 of the narrow tile; 1024 queries: 1.94 -> 1.88 ms, 512: 1.015 -> 1.00; tools/probe/sample_route_probe.py)
    static const int sample_narrow_maxq = lb_tunable("LB_TALL_SAMPLE_NARROW_MAXQ", 384);
    auto candidates = [&](int64_t b, int64_t e, const uint32_t *rowmap, bool boot) {
        if (w->ctx && !boot) LB_HIP(hipStreamSynchronize(s)); // a cancellable call waits for the work in front of every corpus pass
        ctx_check(w->ctx);
        ProfScope p(w, s, prof, 0);
        if (use_narrow)
            launch_gemm_filter_narrow(metric, gx, h->d_norm2.get(), h->d_rnorm.get(), b, e, h->dim, gq, nq, mask, rowmap,
                                      w->cs, boot, s, tile64);
        else if (use_tall16 && h->dim % 32 != 0 && (rowmap || mask) && !entries_pos)
            // the sample of a search over the fp16 copy when the dimension is not a multiple of 32: the f32 tile takes any
            launch_gemm_filter(metric, h->d_X, h->d_norm2.get(), h->d_rnorm.get(), b, e, h->dim, d_q, nq, mask, rowmap, w->cs, boot, s);
        else if (boot && (wsplit == 2 || wsplit == 3) && narrow_ok && !entries_pos && !own_keys &&
                 !(use_tall16 && nq > sample_narrow_maxq))
            // the 8192-row sample of a tall-tile search: the 64-query tile of the narrow kernel (same contraction, f32
            // operands) gets through its 24 K-steps of 32 in 31-35 us, the tall tile through its 48 of 16 in 57
            // (narrow_ok: that kernel reads the f32 queries in 16-B pieces -- a batch pointer that is not 16-B aligned stays
            // on the fp16 kernel below, which reads its own image of the batch)
            launch_gemm_filter_narrow(metric, h->d_X, h->d_norm2.get(), h->d_rnorm.get(), b, e, h->dim, d_q, nq, mask, rowmap, w->cs,
                                      true, s, /*tile64=*/true);
        else if (use_tall16)
            launch_gemm_filter_tall16(metric, h->d_X, knorm2, h->d_rnorm.get(), b, e, h->dim, w->d_qh.get(), d_qinv, nq,
                                      mask, rowmap, w->cs, boot, s, have_xh ? h->d_Xh.get() : nullptr, h->xh_cap, 0u, d_qnrm, kb.gsum,
                                      (tauin && !boot && b == 0 && e == sp.span) ? &tin : nullptr);
        else if (use_tall2)
            launch_gemm_filter_tall2(metric, gx, h->d_norm2.get(), h->d_rnorm.get(), b, e, h->dim, w->d_qs.get(), nq, mask, rowmap, w->cs,
                                     boot, wsplit, s);
        else
            launch_gemm_filter(metric, gx, h->d_norm2.get(), h->d_rnorm.get(), b, e, h->dim, gq, nq, mask, rowmap, w->cs, boot, s);
    };
    int64_t pos = 0;
    int step = 0;
    uint32_t fused_epoch = tin_epoch; // (a wait inside a launch that gave up is reported through one pinned word, whichever launch it was)
    if (sp.on) { // sampled threshold, then one pass over the span (see sample_plan)
        if (sample == SAMPLE_FUSED) {
            const uint32_t *smap = sample_map(h, w, s, rv, sp);
            ProfScope p(w, s, prof, 0);
            FusedSample fs;
            fs.smap = smap;
            fs.count = sp.count;
            fs.m = sp.m;
            fs.ticket = w->d_fsync.get();
            fs.ticket_base = w->fs_base;
            fs.ready = w->d_fsync.get() + 1;
            fs.epoch = w->next_epoch();
            fs.qna = norm_riders ? w->d_qna.get() : nullptr;
            fs.order = order;
            fs.fail_host = w->h_fail.get();
            launch_gemm_filter_narrow_fused(metric, gx, h->d_norm2.get(), h->d_rnorm.get(), 0, sp.span, h->dim, gq, nq, mask, rv.rowmap,
                                            w->cs, s, tile64, fs);
            w->fs_base += fused_sample_blocks(sp.count, nq, tile64);
            fused_epoch = fs.epoch;
        } else {
            if (sample == SAMPLE_GRANULE) {
                ctx_check(w->ctx);
                ProfScope p(w, s, prof, 1); // (timing class "select": threshold work, so that class "gemm" is the corpus pass alone)
                launch_gemm_filter_tall16(metric, h->d_X, knorm2, h->d_rnorm.get(), 0, sp.count, h->dim, w->d_qh.get(), d_qinv,
                                          nq, nullptr, rv.rowmap, w->cs, /*boot=*/true, s, have_xh ? h->d_Xh.get() : nullptr, h->xh_cap,
                                          (uint32_t)(sp.span / (int64_t)(sp.count / 16)), d_qnrm, kb.gsum);
            } else if (sample == SAMPLE_MAPPED) {
                candidates(0, sp.count, sample_map(h, w, s, rv, sp), /*boot=*/true);
            }
            {   // (LIGHT: the scores of the wave-per-row kernel) the thresholds -- unless the pass takes them itself (TAUIN)
                ProfScope p(w, s, prof, 1);
                if (sample == SAMPLE_LIGHT) {
                    const SamplePrep sprep{w->d_qh.get(), d_qinv, dot_lb ? d_qnrm : nullptr, kcenter, tauin, d_qrho, kb.rho_gain};
                    with_rows(h, [&](auto X) {
                        launch_sample_scores(metric, order, X, h->dim, sp.span, sp.count, rv.rowmap, mask, d_q, nullptr, nq, w->cs, nullptr,
                                             s, knorm2, h->d_rnorm.get(), kcenter, prep_rides ? &sprep : nullptr);
                    });
                }
                if (!tauin) launch_sample_tau(w->cs, nullptr, nq, sp.count, sp.m, false, s, d_q, h->dim, norm_riders ? w->d_qna.get() : nullptr, order);
            }
            candidates(0, sp.span, rv.rowmap, /*boot=*/false);
        }
        // (one span covers the view: the finish launch prunes the raw list itself -- everything below tau is in it)
        if (sp.span < n) {
            ProfScope p(w, s, prof, 1);
            launch_select(w->cs, nullptr, nq, kc, 0u, s, (uint32_t)kc, nullptr, false, /*unsorted=*/true);
        }
        pos = sp.span;
        step = 1;
    }
    while (pos < n) {
        const int64_t end = chunk_end_host(step, pos, n, kc, w->cap, false);
        const bool boot = step == 0;
        candidates(pos, end, rv.rowmap, boot);
        {
            ProfScope p(w, s, prof, 1);
            launch_select(w->cs, nullptr, nq, kc, boot ? (uint32_t)(end - pos) : 0u, s, 0u, nullptr, false, /*unsorted=*/true);
        }
        pos = end;
        step++;
    }
    {
        ProfScope p(w, s, prof, 2);
        // members a query may have: twice the results wanted, at least 1024 (the lists hold up to cap entries below tau)
        const uint32_t smax = std::min<uint32_t>(kFinishSmaxMax, std::max<uint32_t>(1024u, 2u * next_pow2_host((uint32_t)k)));
        with_rows(h, [&](auto X) {
            launch_finish(metric, order, X, h->dim, d_q, nq, w->d_qna.get(), w->cs, k, ckeys ? h->d_cstats.get() : h->d_maxnorm2.get(), kb.gamma, finish_beta,
                          h->has_ids ? h->d_ids.get() : nullptr, entries_pos ? rv.rowmap : nullptr, d_dist, d_lab, s, w->h_flags.get(), w->d_done.get(),
                          w->d_xcnt.get(), w->d_xscratch.get(), kFinishSplitMaxQ, smax, kcenter, dot_lb ? h->d_norm2.get() : nullptr, d_qnrm, kb.gsum,
                          dot_lb ? nullptr : d_qrho, kb.qrho_k);
        });
    }
    const int nbad = collect_flagged(w, s, nq, 3u | 4u, nullptr, 0, bad, /*on_host=*/true);
    gave_up = fused_epoch != 0 && (*w->h_fail.get() == fused_epoch || g_fused_fail_next.exchange(0) != 0);
    if (!gave_up) return nbad;
    // a wait inside the fused launch gave up (its workgroups were not co-resident): every query goes the exact way,
    // and the ticket counter is re-based in case the launch did not run to completion
    h->fused_giveups.fetch_add(1);
    LB_HIP(hipMemsetAsync(w->d_fsync.get(), 0, sizeof(uint32_t), s));
    w->fs_base = 0;
    return nq;
}

// A batch of queries of an f32 or fp16 index.  Path selection: <= 4 queries the exact scan (0.50-0.55 ms at 1M x 768); from 5
// queries a candidate route picked by choose_route's cost model (narrow / tall / tall2 / fp16 / f32 tile), exact re-rank behind
// every one of them.  A batch the route leaves unproven is redone (the recovery at the end of the loop); what is unproven after
// that takes the exact scan and is counted in `fallbacks`.
int search_batch_device(lb_gpu_index *h, Workspace *w, hipStream_t s, int nq, const float *d_q, int k,
                        float *d_dist, int64_t *d_lab, int kc_in, bool prof, int64_t &fallbacks)
{
    static const int narrow_min = lb_tunable("LB_NARROW_MINQ", 5);
    static const int f16_kc_mult = lb_tunable("LB_F16_KC_MULT", 0);
    // the same for every attempt (the caller holds the index's shared lock)
    const IndexRowView rv = row_view(h, w);
    const int64_t n = rv.n; // positions to walk: corpus rows, or the visible-row list under a selective filter
    const int cmode = h->cand_mode.load();
    const bool narrow_ok = !h->f16_rows && h->dim % 32 == 0 && ((reinterpret_cast<uintptr_t>(d_q) & 15) == 0);
    // (the fp16 image serves unfiltered searches and searches over a row list -- the persistent kernels gather out of it,
    // dimensions from 256; under a per-row mask test the kernel stages f32 rows)
    const bool have_xh = h->d_Xh && h->xh_rows == h->n && !rv.mask && (!rv.rowmap || h->dim >= 256) &&
                         // (a centred image -- L2 -- is only ever read by the persistent kernels: nothing else knows the centre;
                         // fp16 rows: only the persistent kernels read nothing but the image -- the one-tile form stages f32 rows)
                         ((!h->xh_centred && !h->f16_rows) || tall16_runs_persistent(h->dim, nq, true, rv.rowmap != nullptr, false));
    const bool centred = have_xh && h->xh_centred; // L2 keys about the image's centre (sync_f16_image)
    const bool have_image = h->d_Xs && h->xs_rows == h->n && h->dim % 32 == 0;
    const int kc_max = (int)(w->cap / 4);
    ProfScope whole(w, s, prof, 4);
    bool allow_f16 = true;
    for (int attempt = 0;;) {
        ctx_check(w->ctx);
        // ---- path and route: re-decided by every attempt ----
        // within the fp16 contraction's range: the centred norms when the image is centred, the rows' own norms otherwise
        bool f16_range_ok = centred ? h->xh_c_ok : h->f16_ok;
        // Mid-size corpora and views (below 262,144 rows: offered the fp16 routes since round 4): only while ONE sampled span covers
        // the view with the candidate list the fp16 keys need (twice / four times the split tiles') -- with k = 300 that list is a
        // quarter of the lists' capacity, the sampled span ends short of 200k rows and the rest runs the classic schedule:
        // 0.45 ms where the split tiles over the f32 rows take 0.15.  (Larger corpora: as before.)
        if (cmode == LB_CAND_AUTO && n < 262144 && kc_in > 0) {
            const SamplePlan sp16 = sample_plan(n, f16_kc(kc_in, h->dim, w->cap), w->cap);
            if (!(sp16.on && sp16.span >= n)) f16_range_ok = false;
        }
        // the route over the fp16 copy is on offer (dimensions that are not multiples of 32 included: the MFMA tiles over f32 rows
        // do not apply, the fp16 copy does)
        const bool copy_ok = have_xh && f16_range_ok && allow_f16 &&
                             (cmode == LB_CAND_F16 || (cmode == LB_CAND_AUTO && h->f16_skip.load(std::memory_order_relaxed) == 0));
        // 1 .. 4 queries: the exact scan streams the f32 corpus (0.52 ms per 1M x 768); with the fp16 copy the candidate pass
        // streams half the bytes and the exact re-rank of 512 candidates costs 0.03 ms -- taken when the model says it is cheaper
        bool small_on_copy = false;
        if (!h->nonfinite && nq < narrow_min && copy_ok) {
            const double scan_ms = 0.04 + 1e-6 * (double)n * ((double)h->dim * 0.00066 * (h->f16_rows ? 0.5 : 1.0) + 0.04); // (0.04: sample,
                                                                                                                           // thresholds, select + emit)
            small_on_copy = cmode == LB_CAND_F16 || narrow16_ms(n, h->dim, nq) < scan_ms;
        }
        // the exact scan: rows with inf / NaN components (the MFMA pipeline's keys and error bounds assume finite data; the scan
        // orders non-finite distances canonically, NaN last), an fp16 index without the image route on offer (no image, rows out
        // of fp16's key range, a masked search, the batch beyond the persistent kernels: the exact scan over the fp16 rows, the
        // floor), batches too small for a candidate route -- and an fp16 index's batch that choose_route offers nothing
        const bool scan = h->nonfinite || (h->f16_rows && !copy_ok) ||
                          (nq < ((narrow_ok || copy_ok) ? narrow_min : kGemmMinQ) && !small_on_copy);
        Route route{0, 0, 0.0};
        if (!scan) {
            bool f16_offer = f16_range_ok && allow_f16;
            if (f16_offer && cmode == LB_CAND_AUTO && h->f16_skip.load(std::memory_order_relaxed) > 0) {
                h->f16_skip.fetch_sub(1, std::memory_order_relaxed);
                f16_offer = false;
            }
            // (offset-dominated L2 data: only the centred image's keys resolve anything; dot product over rows of very different
            // lengths: only the lower-bound keys do)
            const bool keys_matter = (centred && h->xh_offset_dom) || (h->metric == LB_METRIC_DOT && h->norm_spread);
            const int cmode_route = (cmode == LB_CAND_AUTO && keys_matter && f16_offer) ? LB_CAND_F16 : cmode;
            route = choose_route(nq, n, h->dim, cmode_route, narrow_ok, have_image, f16_offer, have_xh, !h->f16_rows);
        }
        if (route.kind == 0) {
            h->last_route.store(0, std::memory_order_relaxed); // (lb_debug_last_route keeps the last candidate route)
            scan_with_retry(h, w, s, d_q, nq, nullptr, k, d_dist, d_lab, prof);
            return LB_OK;
        }
        note_route(h, route.kind * 10 + route.split);
        if (attempt == 0 && h->kc_hint_left.load(std::memory_order_relaxed) > 0) { // (the widened-list hint, below)
            h->kc_hint_left.fetch_sub(1, std::memory_order_relaxed);
            kc_in = std::max(kc_in, std::min(h->kc_hint.load(std::memory_order_relaxed), kc_max));
        }
        // candidates kept per query: the fp16 single-product route keeps more (f16_kc)
        const int kc = route.split == 3 ? f16_kc(kc_in, h->dim, w->cap, f16_kc_mult) : kc_in;
        std::vector<int> bad;
        bool gave_up = false;
        const int nbad = run_batch(h, w, s, nq, d_q, k, d_dist, d_lab, prof, route, kc, narrow_ok, have_xh, bad, gave_up);

        // ---- recovery ----
        // More than a handful of unproven queries (each would cost an exact scan of the corpus: 0.5 ms per group of 8 at
        // 1M x 768) and the batch is redone instead, cheapest remedy first:
        //   1. the same route keeping FOUR TIMES the candidates (up to three times over, capped at a quarter of the list) -- the
        //      usual cause is a tight cluster (hundreds of rows whose distances differ by less than the keys resolve): once the
        //      whole cluster is inside the list, the gap to the first row outside it is wide and the proof goes through
        //      (1M x 768 in clusters of ~1000: 1024 queries 93 ms -> a few ms);
        //   2. (fp16 keys) the split-bf16 route, ~100x finer keys, with the widened list;
        //   3. the exact scan for what is still unproven.
        const bool can_widen = attempt <= 2 && kc < kc_max && (int64_t)kc * 2 < n; // (up to three widenings: x4, x16, x64, capped)
        if (route.split == 3 && cmode == LB_CAND_AUTO && attempt <= 3 && !(nbad > 8 && can_widen)) {
            if (nbad * 8 > nq) { // the fp16 keys are too coarse for this data even with the widened list: leave the route alone
                const int span = h->f16_span.load(); // for a while (doubling spans)
                h->f16_skip.store(span);
                h->f16_span.store(std::min(span * 2, 4096));
            } else if (nbad == 0) {
                h->f16_span.store(16);
            }
        }
        if (attempt >= 1 && attempt <= 3 && nbad <= 8) { // the widened list proved the batch: start the next searches there
            h->kc_hint.store(kc_in, std::memory_order_relaxed);
            h->kc_hint_left.store(256, std::memory_order_relaxed);
        }
        if (nbad > 8 && !gave_up && attempt < 4) {
            if (can_widen) { // 1.
                kc_in = std::min(kc_in * 4, kc_max);
                attempt++;
                continue;
            }
            if (route.split == 3 && allow_f16) { // 2. (one attempt, numbered 4: nothing follows it but the scan)
                allow_f16 = false;
                attempt = 4;
                continue;
            }
        }
        if (nbad > 0) { // 3.
            fallbacks += nbad;
            scan_with_retry(h, w, s, d_q, nq, gave_up ? nullptr : &bad, k, d_dist, d_lab, prof);
        }
        return LB_OK;
    }
}

void finish_profile(lb_gpu_index *h, Workspace *w)
{
    float ms[5] = {0, 0, 0, 0, 0};
    int cnt[5] = {0, 0, 0, 0, 0};
    for (size_t i = 0; i < w->ev_used; i++) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, w->events[i].a, w->events[i].b) == hipSuccess) {
            ms[w->events[i].cls] += t;
            cnt[w->events[i].cls]++;
        }
    }
    w->ev_used = 0;
    std::lock_guard<std::mutex> g(h->prof_mu);
    for (int i = 0; i < 5; i++) {
        h->prof_ms[i] = ms[i];
        h->prof_n[i] = cnt[i];
    }
}

// What a search entry point answers before it touches the device, in this order: LB_ERR_INVALID_ARG, a call of another element
// type than the index's, LB_OK for no queries (neither k nor the context is looked at), k beyond LB_MAX_K, the context.
int search_args(lb_gpu_index *h, int64_t nq, const void *queries, int k, const void *dist, const void *labels, const lb_cancel *ctx, int dtype)
{
    if (h && nq == 0 && k > 0) return dtype_mismatch(h, dtype);
    return knn_args(h, nq, queries, k, dist, labels, ctx, [&] { return dtype_mismatch(h, dtype); });
}

// ---- a row bitmap given with the call (lb_gpu_index_search*_bitmap*) ------------------------------------------------------------
// The bitmap as an entry point got it: host or device memory, one bit per row position, least significant bit first; bits null:
// the plain search.  lease: where a host bitmap's bytes go on the device -- the entry point's, declared outside every guard, so
// that the stream is drained before the bytes return to the pool.
struct CallBits {
    const uint8_t *bits = nullptr;
    int64_t nbits = 0;
    bool on_device = true;
    Lease *lease = nullptr;
};

// The view of a call from its bitmap (kernels_index_call.hip), on the call's stream and into the call's workspace: the bits ANDed
// with the handle's effective mask, the ascending list of the rows that pass, and their number -- the four bytes and the one
// synchronisation the build costs.  From that number rebuild_rowmap's rule, with the same LB_ROWMAP_MAX_PCT: the list at or
// below it, the per-row test of the call's mask above it, and the unmasked view when nothing is hidden at all.  The caller holds
// the shared lock and has checked nbits == h->n >= 1; the handle is only read (d_mask, has_mask).
void build_call_view(lb_gpu_index *h, Workspace *w, hipStream_t s, const CallBits &b, bool prof)
{
    static const int max_pct = lb_tunable("LB_ROWMAP_MAX_PCT", 95);
    const int64_t n = h->n, blocks = index_call_blocks(n);
    const uint8_t *d_bits = b.bits;
    if (!b.on_device) {
        const size_t bytes = (size_t)((n + 7) / 8);
        b.lease->reset(h->device, bytes);
        LB_HIP(hipMemcpyAsync(b.lease->p, b.bits, bytes, hipMemcpyHostToDevice, s));
        d_bits = b.lease->as<uint8_t>();
    }
    w->d_cmask.ensure((size_t)blocks * INDEX_CALL_BLOCK_ROWS);
    w->d_crows.ensure((size_t)n);
    w->d_cscratch.ensure((size_t)compact_scratch_words(n));
    if (!w->h_ctotal) w->h_ctotal.alloc(1);
    {
        ProfScope p(w, s, prof, 1);
        launch_index_call_bits(d_bits, h->has_mask ? h->d_mask.get() : nullptr, n, w->d_cmask.get(), w->d_cscratch.get(), s);
    }
    {
        ProfScope p(w, s, prof, 1);
        launch_compact_offsets(w->d_cscratch.get(), blocks, s);
    }
    {
        ProfScope p(w, s, prof, 1);
        launch_index_call_scatter(w->d_cmask.get(), n, w->d_cscratch.get(), w->d_crows.get(), s);
    }
    LB_LAUNCH_CHECK();
    LB_HIP(hipMemcpyAsync(w->h_ctotal.get(), w->d_cscratch.get() + blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    const int64_t visible = (int64_t)*w->h_ctotal.get();
    if (max_pct > 0 && visible * 100 <= n * (int64_t)max_pct) w->cv = IndexRowView{nullptr, w->d_crows.get(), visible};
    else if (visible == n && !h->has_mask) w->cv = IndexRowView{nullptr, nullptr, n};
    else w->cv = IndexRowView{w->d_cmask.get(), nullptr, n};
    w->call_view = true;
}

// A search's workspace: it goes back to the pool when the call ends, unless the call dropped it.
struct WsLoan {
    lb_gpu_index *h;
    std::unique_ptr<Workspace> w;
    ~WsLoan()
    {
        if (!w) return;
        w->ctx = nullptr;
        w->call_view = false;
        release_ws(h, std::move(w));
    }
};

} // namespace

extern "C" {

int64_t lb_gpu_index_last_fallbacks(const lb_gpu_index *h) { return h ? h->last_fallbacks.load() : 0; }
int64_t lb_gpu_index_fused_giveups(const lb_gpu_index *h) { return h ? h->fused_giveups.load() : 0; }
int lb_gpu_index_last_route(const lb_gpu_index *h) { return h ? h->last_route.load() : 0; }

static int search_device(lb_gpu_index *h, int64_t nq, const void *d_queries, int k, float *d_dist, int64_t *d_labels, void *stream,
                         const lb_cancel *ctx, int dtype, const CallBits &call = CallBits{})
{
    int rc = search_args(h, nq, d_queries, k, d_dist, d_labels, ctx, dtype);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(h->mu);
    if (call.bits && call.nbits != h->n) { // (set_filter's n != ntotal rule)
        h->set_error("a bitmap of %lld bits for %lld rows", (long long)call.nbits, (long long)h->n);
        return LB_ERR_INVALID_ARG;
    }
#ifdef LB_DIAG
    if (g_search_fail_next.exchange(0) != 0) { h->set_error("search failure forced by lb_debug_search_fail_next"); return LB_ERR_INTERNAL; }
#endif
    WsLoan loan{h, nullptr};
    int kc = 0;
    rc = guard(h, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        uint32_t cap;
        cand_geometry(k, kc, cap);
        loan.w = acquire_ws(h, (int)std::min<int64_t>(nq, kMaxBatch), cap);
        return LB_OK;
    });
    if (rc != LB_OK) return rc;
    Workspace *w = loan.w.get();
    hipStream_t s = stream ? (hipStream_t)stream : w->stream;
    rc = guard(h, s, [&]() -> int {
        const bool prof = h->profiling.load() != 0;
        w->ev_used = 0;
        w->ctx = ctx;
        int64_t fallbacks = 0;
        if (h->n == 0) {
            launch_fill_empty(d_dist, d_labels, nq * k, s);
        } else {
            if (call.bits) { // the call's view, once for all its batches
                ctx_check(ctx);
                build_call_view(h, w, s, call, prof);
            }
            for (int64_t q0 = 0; q0 < nq; q0 += kMaxBatch) {
                const int bq = (int)std::min<int64_t>(kMaxBatch, nq - q0);
                const float *bq_f32 = nullptr;
                if (dtype != 0) { // fp16 / int8 queries: widened exactly into the workspace's f32 batch, then searched as any other
                    w->d_q.ensure((size_t)bq * h->dim);
                    if (dtype == 2)
                        launch_widen_i8(static_cast<const int8_t *>(d_queries) + (size_t)q0 * h->dim, w->d_q.get(), (int64_t)bq * h->dim, s);
                    else
                        launch_widen_f16(static_cast<const uint16_t *>(d_queries) + (size_t)q0 * h->dim, w->d_q.get(), (int64_t)bq * h->dim, s);
                    bq_f32 = w->d_q.get();
                } else {
                    bq_f32 = static_cast<const float *>(d_queries) + (size_t)q0 * h->dim;
                }
                const int brc = h->i8_rows ? search_batch_i8(h, w, s, bq, bq_f32, static_cast<const int8_t *>(d_queries) + (size_t)q0 * h->dim, k,
                                                             d_dist + (size_t)q0 * k, d_labels + (size_t)q0 * k, prof)
                                           : search_batch_device(h, w, s, bq, bq_f32, k, d_dist + (size_t)q0 * k, d_labels + (size_t)q0 * k,
                                                                 kc, prof, fallbacks);
                if (brc != LB_OK) return brc;
            }
        }
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        h->last_fallbacks.store(fallbacks);
        if (prof) finish_profile(h, w);
        return LB_OK;
    });
    if (rc == LB_ERR_CANCELLED || rc == LB_ERR_DEADLINE) {
        // The context stopped the enqueuing and guard() let what was already on the stream finish (it writes into the caller's
        // buffers, which hold unspecified values as after any failed call).  A fused launch may have been skipped between its
        // host-side bookkeeping and the device: re-base the ticket
        (void)hipGetLastError();
        w->ev_used = 0;
        (void)hipMemsetAsync(w->d_fsync.get(), 0, sizeof(uint32_t), s);
        (void)hipStreamSynchronize(s);
        w->fs_base = 0;
    } else if (rc == LB_ERR_HIP || rc == LB_ERR_OOM || rc == LB_ERR_INTERNAL) {
        loan.w.reset(); // what the workspace holds on the device is unknown: it is freed, not pooled
    }
    return rc;
}

int lb_gpu_index_search_device_ctx(lb_gpu_index *h, int64_t nq, const float *d_queries, int k, float *d_dist,
                                   int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return search_device(h, nq, d_queries, k, d_dist, d_labels, stream, ctx, 0);
}
int lb_gpu_index_search_f16_device_ctx(lb_gpu_index *h, int64_t nq, const uint16_t *d_queries, int k, float *d_dist,
                                       int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return search_device(h, nq, d_queries, k, d_dist, d_labels, stream, ctx, 1);
}
int lb_gpu_index_search_i8_device_ctx(lb_gpu_index *h, int64_t nq, const int8_t *d_queries, int k, float *d_dist,
                                      int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return search_device(h, nq, d_queries, k, d_dist, d_labels, stream, ctx, 2);
}

int lb_gpu_index_search_device(lb_gpu_index *h, int64_t nq, const float *d_queries, int k, float *d_dist,
                               int64_t *d_labels, void *stream)
{
    return lb_gpu_index_search_device_ctx(h, nq, d_queries, k, d_dist, d_labels, stream, nullptr);
}

lb_cancel *lb_cancel_new(void) { return new (std::nothrow) lb_cancel(); }
void lb_cancel_free(lb_cancel *c) { delete c; }
void lb_cancel_fire(lb_cancel *c) { if (c) c->fired.store(1); }
void lb_cancel_set_deadline_ms(lb_cancel *c, int64_t ms_from_now)
{
    if (!c) return;
    if (ms_from_now < 0) { c->deadline_ns.store(0); return; }
    const long long now = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    long long d = now + (long long)ms_from_now * 1000000ll;
    if (d == 0) d = 1;
    c->deadline_ns.store(d);
}
int lb_cancel_state(const lb_cancel *c) { return ctx_state(c); }

// Host-pointer search of one or several requests with the same k as ONE device batch: borrowed host buffers -> pooled pinned
// slab -> HBM (async DMA on the call's own stream), and back; every request gets its rows of the result.
// (dtype: the requests' queries are fp16 -- 2 bytes an element -- or int8 -- 1 byte; those are never combined)
// (call: the row bitmap of a call that brought one -- such a call is one request, never combined)
static int host_search_multi(lb_gpu_index *h, HostReq *const *reqs, int nreq, int k, const lb_cancel *ctx, int dtype = 0,
                             const CallBits &call = CallBits{})
{
    int64_t nq = 0;
    for (int i = 0; i < nreq; i++) nq += reqs[i]->nq;
    // (before any staging is sized: nq * k * 12 bytes of pinned + device memory per call; the caller has answered k)
    if (nq > ((int64_t)1 << 40) / ((int64_t)h->dim + 3 * (int64_t)k)) { h->set_error("batch too large"); return LB_ERR_INVALID_ARG; }
    const HostSlab sl(nq, (size_t)h->dim * h->elem_bytes(), k);
    std::unique_ptr<HostStage> st;
    return guard(h, nullptr, [&]() -> int { // (the staging is the call's own, not pooled while it is in use: nothing to drain for)
        LB_HIP(hipSetDevice(h->device));
        {
            std::lock_guard<std::mutex> g(h->ws_mu);
            for (size_t i = 0; i < h->hs_free.size(); i++)
                if (h->hs_free[i]->d_buf.count() >= sl.total) {
                    st = std::move(h->hs_free[i]);
                    h->hs_free.erase(h->hs_free.begin() + (long)i);
                    break;
                }
        }
        if (!st) {
            st = std::make_unique<HostStage>();
            st->device = h->device;
            LB_HIP(hipStreamCreateWithFlags(&st->stream.h, hipStreamNonBlocking));
            st->d_buf.alloc(std::max<size_t>(sl.total, 1u << 20));
            st->h_buf.alloc(st->d_buf.count());
        }
        char *hb = st->h_buf.get(), *dbuf = st->d_buf.get();
        sl.gather(reqs, nreq, hb);
        LB_HIP(hipMemcpyAsync(dbuf, hb, sl.qb, hipMemcpyHostToDevice, st->stream));
        // (direct results: the search's own stream synchronisation is what makes them visible; large ones go through HBM and one DMA)
        char *obuf = sl.direct ? hb : dbuf;
        const int rc = search_device(h, nq, dbuf, k, reinterpret_cast<float *>(obuf + sl.doff), reinterpret_cast<int64_t *>(obuf + sl.loff),
                                     st->stream, ctx, dtype, call);
        if (rc == LB_OK) {
            if (!sl.direct) {
                LB_HIP(hipMemcpyAsync(hb + sl.doff, dbuf + sl.doff, sl.db + sl.lb, hipMemcpyDeviceToHost, st->stream));
                LB_HIP(hipStreamSynchronize(st->stream));
            }
            sl.scatter(reqs, nreq, hb, k);
        }
        std::lock_guard<std::mutex> g(h->ws_mu);
        if (h->hs_free.size() < 8) h->hs_free.push_back(std::move(st));
        return rc;
    });
}

// the host-pointer entry points; dtype: the element type of `queries` (0 float32, 1 fp16 bits, 2 int8: host_search_multi copies bytes)
static int host_search(lb_gpu_index *h, int64_t nq, const void *queries, int k, float *dist, int64_t *labels, const lb_cancel *ctx, int dtype,
                       const CallBits &call = CallBits{})
{
    if (h && nq == 0 && k > 0) return LB_OK; // (a host call of no queries does not look at the index's element type either)
    // (without the context: a host call answers it after the size of its batch, in the device search)
    if (const int rc = search_args(h, nq, queries, k, dist, labels, nullptr, dtype)) return rc;
    // (a call with a cancellation context is searched on its own: its deadline is not its neighbours'; fp16 and int8 calls too)
    HostReq me{static_cast<const float *>(queries), nq, dist, labels, k};
    // (and a call with a row bitmap of its own: its view is not its neighbours')
    if (dtype == 0 && !ctx && !call.bits && nq <= SearchCombiner::kMaxNq && h->combiner.on.load() != 0)
        return h->combiner.search(me, [h](HostReq *const *reqs, int n, int kk) { return host_search_multi(h, reqs, n, kk, nullptr); });
    HostReq *one = &me;
    return host_search_multi(h, &one, 1, k, ctx, dtype, call);
}

int lb_gpu_index_search_ctx(lb_gpu_index *h, int64_t nq, const float *queries, int k, float *dist, int64_t *labels,
                            const lb_cancel *ctx)
{
    return host_search(h, nq, queries, k, dist, labels, ctx, 0);
}
int lb_gpu_index_search_f16_ctx(lb_gpu_index *h, int64_t nq, const uint16_t *queries, int k, float *dist, int64_t *labels,
                                const lb_cancel *ctx)
{
    return host_search(h, nq, queries, k, dist, labels, ctx, 1);
}
int lb_gpu_index_search_f16(lb_gpu_index *h, int64_t nq, const uint16_t *queries, int k, float *dist, int64_t *labels)
{
    return lb_gpu_index_search_f16_ctx(h, nq, queries, k, dist, labels, nullptr);
}
int lb_gpu_index_search_i8_ctx(lb_gpu_index *h, int64_t nq, const int8_t *queries, int k, float *dist, int64_t *labels,
                               const lb_cancel *ctx)
{
    return host_search(h, nq, queries, k, dist, labels, ctx, 2);
}
int lb_gpu_index_search_i8(lb_gpu_index *h, int64_t nq, const int8_t *queries, int k, float *dist, int64_t *labels)
{
    return lb_gpu_index_search_i8_ctx(h, nq, queries, k, dist, labels, nullptr);
}

// the same searches under a row bitmap given with the call (include/longbow_gpu.h, "call bitmap"); a NULL bitmap: the plain search
// through the plain path.  The host forms' bitmap bytes travel in `bits`, declared here, outside every guard.
static int host_search_bitmap(lb_gpu_index *h, int64_t nq, const void *queries, int k, const uint8_t *bitmap, int64_t nbits, float *dist,
                              int64_t *labels, const lb_cancel *ctx, int dtype)
{
    if (!bitmap) return host_search(h, nq, queries, k, dist, labels, ctx, dtype);
    Lease bits;
    return host_search(h, nq, queries, k, dist, labels, ctx, dtype, CallBits{bitmap, nbits, false, &bits});
}
int lb_gpu_index_search_bitmap_ctx(lb_gpu_index *h, int64_t nq, const float *queries, int k, const uint8_t *bitmap, int64_t nbits,
                                   float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return host_search_bitmap(h, nq, queries, k, bitmap, nbits, dist, labels, ctx, 0);
}
int lb_gpu_index_search_f16_bitmap_ctx(lb_gpu_index *h, int64_t nq, const uint16_t *queries, int k, const uint8_t *bitmap, int64_t nbits,
                                       float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return host_search_bitmap(h, nq, queries, k, bitmap, nbits, dist, labels, ctx, 1);
}
int lb_gpu_index_search_i8_bitmap_ctx(lb_gpu_index *h, int64_t nq, const int8_t *queries, int k, const uint8_t *bitmap, int64_t nbits,
                                      float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return host_search_bitmap(h, nq, queries, k, bitmap, nbits, dist, labels, ctx, 2);
}
int lb_gpu_index_search_bitmap_device_ctx(lb_gpu_index *h, int64_t nq, const float *d_queries, int k, const uint8_t *d_bitmap,
                                          int64_t nbits, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return search_device(h, nq, d_queries, k, d_dist, d_labels, stream, ctx, 0, CallBits{d_bitmap, nbits, true, nullptr});
}
int lb_gpu_index_search_f16_bitmap_device_ctx(lb_gpu_index *h, int64_t nq, const uint16_t *d_queries, int k, const uint8_t *d_bitmap,
                                              int64_t nbits, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return search_device(h, nq, d_queries, k, d_dist, d_labels, stream, ctx, 1, CallBits{d_bitmap, nbits, true, nullptr});
}
int lb_gpu_index_search_i8_bitmap_device_ctx(lb_gpu_index *h, int64_t nq, const int8_t *d_queries, int k, const uint8_t *d_bitmap,
                                             int64_t nbits, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return search_device(h, nq, d_queries, k, d_dist, d_labels, stream, ctx, 2, CallBits{d_bitmap, nbits, true, nullptr});
}

int lb_gpu_index_set_search_combining(lb_gpu_index *h, int enable) { return combining_set(h, enable); }
int lb_gpu_index_combining_stats(const lb_gpu_index *h, int64_t out[2]) { return combining_stats(h, out); }

int lb_gpu_index_search(lb_gpu_index *h, int64_t nq, const float *queries, int k, float *dist, int64_t *labels)
{
    return lb_gpu_index_search_ctx(h, nq, queries, k, dist, labels, nullptr);
}

int lb_gpu_index_set_profiling(lb_gpu_index *h, int enable)
{
    if (!h) return LB_ERR_INVALID_ARG;
    h->profiling.store(enable ? 1 : 0);
    return LB_OK;
}

int lb_gpu_index_last_timing(const lb_gpu_index *hc, float ms[5], int n_launch[5])
{
    if (!hc || !ms || !n_launch) return LB_ERR_INVALID_ARG;
    auto *h = const_cast<lb_gpu_index *>(hc);
    std::lock_guard<std::mutex> g(h->prof_mu);
    for (int i = 0; i < 5; i++) { ms[i] = h->prof_ms[i]; n_launch[i] = h->prof_n[i]; }
    return LB_OK;
}

#ifdef LB_DIAG
// Diagnostic build only (python -m longbow_amd.build --diag -> liblongbow_gpu_diag.so; the tests that force a
// fallback path load that library): none of these symbols exists in liblongbow_gpu.so.
// Test hooks (both settings are exact; they only choose between two schedules / expose host logic).
void lb_debug_set_sample_tau(int v) { g_sample_tau.store(v); } // 0: classic bootstrap schedule only
void lb_debug_fused_fail_next(int v) { g_fused_fail_next.store(v); } // the next fused sample launch counts as timed out (-> exact path for the batch)
void lb_debug_tin_withhold_next(int v) { g_tin_withhold_next.store(v); } // the next TAUIN launch's waits give up in the kernel (-> exact path)
int lb_debug_last_route(void) { return g_last_route.load(); } // RouteKind * 10 + split of the most recent batched search
void lb_debug_search_fail_next(int v) { g_search_fail_next.store(v); } // the next search in this process returns LB_ERR_INTERNAL
// host-only: the sampled-threshold plan for a view of n rows (tests check its invariants without a GPU);
// out = {on, span, count, m}
void lb_debug_sample_plan(long long n, int keep, unsigned cap, unsigned count_max, long long *out)
{
    const SamplePlan p = sample_plan((int64_t)n, keep, cap, count_max ? count_max : 8192u);
    out[0] = p.on ? 1 : 0;
    out[1] = p.span;
    out[2] = p.count;
    out[3] = p.m;
}
// host-only: the candidate-list geometry of a request of k (candidates kept per query, list capacity)
void lb_debug_cand_geometry(int k, int *kc, unsigned *cap)
{
    int c;
    uint32_t p;
    cand_geometry(k, c, p);
    *kc = c;
    *cap = p;
}
// counters of the fused launch and of the finish launch (they only observe)
void lb_debug_read_fused_probe(unsigned long long *out, int reset) { lb::read_fused_probe(out, reset != 0); }
void lb_debug_read_finish_probe(unsigned long long *out, int reset) { lb::read_finish_probe(out, reset != 0); }
#endif

} // extern "C"
