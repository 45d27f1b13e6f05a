// pq.hip -- host side of the PQ/ADC entry points of include/longbow_gpu.h.
//
// Codebooks arrive as the reference's own serialised blob
// (internal/pq/persistence.go:9-35) with DeserializePQEncoder's validation
// (persistence.go:38-73).  K must be 256: simd.adcBatchGeneric hard-codes the
// table stride 256 (internal/simd/simd.go:350) while pq.BuildADCTable writes
// stride K (internal/pq/adc_table.go:46); they agree only at K = 256.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_handle.h"

#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

using namespace lb;

namespace {
uint32_t rd_u32le(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
struct PqScratch;
} // namespace

struct lb_gpu_pq : FilteredHandle { // searches and reads share mu; adds, reserve and the filter calls take it alone
    int M = 0, K = 0, sub = 0;
    DevBuf<float> d_codebooks;
    DevBuf<uint8_t> d_codes;
    // per-search scratch (lists, tables, sample and candidate buffers, profiling events) is pooled on the handle: a search
    // must not hipMalloc/hipFree (the latter synchronises the device under every concurrent search)
    std::mutex sc_mu;
    std::vector<std::unique_ptr<PqScratch>> sc_free;
    std::atomic<int> profiling{0}; // instrumentation (bench.py): HIP events around the main code pass and the whole search
    std::atomic<int> prefilter{1}; // 0 = exact f32-table pass only (lb_gpu_pq_set_prefilter; both are exact)
    SearchCombiner combiner;       // concurrent host-pointer searches of a few queries each are combined (lb_host.h)
    // what served the queries of the last COMPLETED device batch (lb_gpu_pq_last_search_stats) and, when it was profiled, the
    // times of its last query (lb_gpu_pq_last_timing): observing only
    mutable std::mutex stats_mu;
    int64_t last_stats[6] = {0, 0, 0, 0, 0, 0};
    float prof_ms[2] = {0.f, 0.f};
};

namespace {
constexpr int kPqMaxK = 4096;        // largest k of a PQ search (the list of a query holds 4 * k entries)
constexpr int64_t kPqMaxNq = 65536;  // queries per call
constexpr uint32_t kCandCap = 65536; // prefilter survivors per query (expected: a few thousand)

// The copy is one hipMemcpy: the peak is old + new (grow_capacity keeps the step small beyond 1 GiB); a caller that knows the
// final size avoids it with lb_gpu_pq_reserve.
void pq_grow(lb_gpu_pq *p, int64_t need)
{
    if (need <= p->capacity) return;
    const int64_t cap = grow_capacity(p->capacity, need, (size_t)p->M);
    DevBuf<uint8_t> nc;
    nc.alloc((size_t)cap * p->M);
    if (p->n > 0) LB_HIP(hipMemcpy(nc.get(), p->d_codes.get(), (size_t)p->n * p->M, hipMemcpyDeviceToDevice));
    p->filter.grow(p->n, cap);
    p->d_codes = std::move(nc);
    p->capacity = cap;
}

// n more rows: fill(dst) enqueues on p->stream whatever writes them at dst; they are committed (p->n) last, once they are
// stored and an active filter's list holds them
template <class Fill> int pq_append(lb_gpu_pq *p, int64_t n, Fill &&fill)
{
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (p->n + n > (int64_t)0xffffffffll) { p->set_error("more than 2^32 codes per device"); return LB_ERR_UNSUPPORTED; }
    if (p->filter.on)
        if (const int st = filter_fits(p, p->n + n)) return st;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        pq_grow(p, p->n + n);
        fill(p->d_codes.get() + (size_t)p->n * p->M);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(p->stream));
        p->filter.on_append(p->n, p->n + n, p->stream);
        p->n += n;
        return LB_OK;
    });
}

int add_codes_impl(lb_gpu_pq *p, int64_t n, const uint8_t *codes, hipMemcpyKind kind)
{
    if (!p || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    return pq_append(p, n, [&](uint8_t *dst) { LB_HIP(hipMemcpyAsync(dst, codes, (size_t)n * p->M, kind, p->stream)); });
}

// What a k-NN entry point answers before it touches the device: INVALID_ARG, nothing to do (the caller returns on nq == 0
// too), the context, then the two limits.  (knn_args of lb_handle.h asks in another order and for LB_MAX_K.)
int pq_knn_args(lb_gpu_pq *p, int64_t nq, const void *queries, int k, const void *dist, const void *labels, const lb_cancel *ctx)
{
    if (!p || nq < 0 || k <= 0 || (nq > 0 && (!queries || !dist || !labels))) return LB_ERR_INVALID_ARG;
    if (nq == 0) return LB_OK;
    if (const int st = ctx_state(ctx)) return ctx_fail(p, st);
    if (k > kPqMaxK) { p->set_error("k=%d exceeds the supported maximum %d", k, kPqMaxK); return LB_ERR_UNSUPPORTED; }
    if (nq > kPqMaxNq) { p->set_error("nq=%lld exceeds %lld queries per call", (long long)nq, (long long)kPqMaxNq); return LB_ERR_UNSUPPORTED; }
    return LB_OK;
}

struct PqScratch {
    int device = 0;
    int nq_cap = 0;
    uint32_t cap = 0;
    int M = 0;
    // the candidate state as the kernels take it (by value): pointers into the four buffers below, filled once (acquire_scratch)
    CandState cs{};
    DevBuf<uint64_t> d_lists, d_tau;
    DevBuf<uint32_t> d_cnt, d_flags;
    DevBuf<float> d_tables;      // [nq][M*256] f32
    DevBuf<uint8_t> d_qtabs;     // [nq][M*256] u8
    DevBuf<float> d_minrng;      // [nq][M][4]: subtable minimum, range, bad flag
    DevBuf<int> d_params;        // [nq][4]
    DevBuf<uint32_t> d_cand;     // [4][kCandCap] survivors of the (up to four) queries in flight
    DevBuf<uint32_t> d_cand_cnt; // [nq]
    DevBuf<int> d_slots;         // 0..nq-1
    DevBuf<uint64_t> d_samp;     // ADC entries of the sampled rows
    PinnedBuf<uint32_t> h_flags;
    EventH ev[4]; // a profiled search: {start, end} of the whole search, {start, end} of the last query's pass over the codes
    ~PqScratch() { (void)hipSetDevice(device); }
};

std::unique_ptr<PqScratch> acquire_scratch(lb_gpu_pq *p, int nq, uint32_t cap, size_t samp_entries)
{
    std::unique_ptr<PqScratch> sc;
    {
        std::lock_guard<std::mutex> g(p->sc_mu);
        for (size_t i = 0; i < p->sc_free.size(); i++)
            if (p->sc_free[i]->nq_cap >= nq && p->sc_free[i]->cap == cap) {
                sc = std::move(p->sc_free[i]);
                p->sc_free.erase(p->sc_free.begin() + (long)i);
                break;
            }
    }
    if (!sc) {
        sc = std::make_unique<PqScratch>();
        sc->device = p->device;
        sc->nq_cap = std::max(nq, 4);
        sc->cap = cap;
        sc->M = p->M;
        sc->cs.cap = cap;
        const size_t nqc = (size_t)sc->nq_cap;
        sc->d_lists.alloc(nqc * cap);
        sc->d_cnt.alloc(nqc);
        sc->d_tau.alloc(nqc);
        sc->d_flags.alloc(nqc);
        sc->cs.lists = sc->d_lists.get();
        sc->cs.cnt = sc->d_cnt.get();
        sc->cs.tau = sc->d_tau.get();
        sc->cs.flags = sc->d_flags.get();
        sc->d_tables.alloc(nqc * p->M * 256);
        sc->d_qtabs.alloc(nqc * p->M * 256);
        sc->d_minrng.alloc(nqc * p->M * 4);
        sc->d_params.alloc(nqc * 4);
        sc->d_cand.alloc((size_t)4 * kCandCap);
        sc->d_cand_cnt.alloc(nqc);
        sc->d_slots.alloc(nqc);
        sc->h_flags.alloc(nqc);
        std::vector<int> slots(nqc);
        for (size_t q = 0; q < nqc; q++) slots[q] = (int)q;
        LB_HIP(hipMemcpy(sc->d_slots.get(), slots.data(), nqc * sizeof(int), hipMemcpyHostToDevice));
    }
    sc->d_samp.ensure(samp_entries);
    return sc;
}

// A search's hold on its scratch.  Declared outside guard() like a Lease: it goes back to the handle's pool on every path
// -- done, cancelled, failed -- once the stream is drained, never to hipFree under the concurrent searches.
struct ScratchLoan {
    lb_gpu_pq *p;
    std::unique_ptr<PqScratch> sc;
    ~ScratchLoan()
    {
        std::lock_guard<std::mutex> g(p->sc_mu);
        if (sc && p->sc_free.size() < 4) p->sc_free.push_back(std::move(sc)); // (lb_gpu_pq_new reserved the room: nothing throws)
    }
};

// Sampled admission threshold (same reasoning as index_search.hip: sample_plan): one row in `stride` is scored
// exactly, the m-th best sample entry becomes tau, and the codes are walked once.  About m*stride rows
// pass (4096 at stride 512); fewer than k or more than the list holds is detected by the select and
// the query is redone by the bootstrap schedule.  Two-level m-th minimum: the sample (195k entries at
// 100M rows) is larger than one list.  Stride 512 with a 16384-entry list (mean + 5 sigma = 11.3k
// admitted rows) instead of stride 256 / 8192 halves the sampling pass (49 -> 25 us at 100M rows).
// samp_count == 0: no sampled pass, the list keeps the `cap` given.  (tests/adc_bound.py: plan() restates this.)
struct SamplePlan { uint32_t samp_count; int samp_m; uint32_t cap; };

SamplePlan sample_plan(int64_t n_vis, int k, uint32_t cap)
{
    if (n_vis >= 65536 && n_vis < ((int64_t)1 << 32)) {
        const uint32_t cap_s = std::max<uint32_t>(16384u, cap);
        const int64_t stride = n_vis >= ((int64_t)8192 * 512) ? 512 : 256;
        const int64_t cnt = std::max<int64_t>(8192, (n_vis + stride - 1) / stride);
        const double lambda = (double)k * (double)cnt / (double)n_vis;
        const int m = std::max(8, (int)std::ceil(lambda + 5.0 * std::sqrt(lambda) + 4.0));
        const double loose = (double)m * ((double)n_vis / (double)cnt) * (1.0 + 5.0 / std::sqrt((double)m));
        // The last condition is launch_sample_topm's own: its groups of 8192 = ST_THREADS * ST_PER entries (kernels_scan.hip)
        // number ceil(cnt / 8192) <= 8192 / m (cnt >= 8192, so at least one), hence groups * m <= 8192 <= 16384 <= cap_s.  A
        // plan made here is never refused there; PqSearch::threshold treats a refusal as an internal error.
        if (m <= 32 && loose <= (double)(cap_s - (uint32_t)k) && cnt <= (int64_t)8192 * (8192 / m)) return {(uint32_t)cnt, m, cap_s};
    }
    return {0, 0, cap};
}

// One device batch: the passes of its queries in the order they are enqueued on s.  Under a row filter the search walks the
// v.n positions of the ascending list of visible rows (kernels_pq_list.hip) instead of the p->n rows: the plan, the chunk
// schedule and the selects count positions, the entries carry rows.
struct PqSearch {
    lb_gpu_pq *p;
    RowView v;
    PqScratch &sc;
    hipStream_t s;
    int nq, k;
    SamplePlan plan;
    bool prefilter, prof; // prefilter: a sampled plan with the byte-table pass on
    EmitArgs em;          // the search's last select writes the k results AND the slot's status word into pinned host memory (no D2H copy)
    int64_t stats[6];     // {sampled plan, four-query pass, two-query pass, single prefilter pass, bootstrap redo, safe redo} (queries)

    const uint8_t *codes() const { return p->d_codes.get(); }
    const float *tab(int q) const { return sc.d_tables.get() + (size_t)q * p->M * 256; }
    uint8_t *qtab(int q) const { return sc.d_qtabs.get() + (size_t)q * p->M * 256; }
    int *prm(int q) const { return sc.d_params.get() + q * 4; }
    uint32_t *cand(int j) const { return sc.d_cand.get() + (size_t)j * kCandCap; } // of the j-th query of the group in flight
    uint32_t *ccnt(int q) const { return sc.d_cand_cnt.get() + q; }
    const int *slot(int q) const { return sc.d_slots.get() + q; }

    // the passes over the rows or, under a filter, over the list
    void exact_scan(int q, int64_t begin, int64_t end, bool boot)
    {
        if (v.rowmap) launch_adc_list_scan(tab(q), p->M, codes(), v.rowmap, begin, end, q, sc.cs, boot, s);
        else launch_adc_scan(tab(q), p->M, codes(), begin, end, q, nullptr, sc.cs, boot, nullptr, 0, s);
    }
    void prefilter_one(int q, int j)
    {
        if (v.rowmap) launch_adc_list_prefilter(qtab(q), prm(q), p->M, codes(), v.rowmap, v.n, cand(j), kCandCap, ccnt(q), s);
        else launch_adc_prefilter(qtab(q), prm(q), p->M, codes(), v.n, cand(j), kCandCap, ccnt(q), s);
    }
    bool prefilter_two(int q, int j) // queries q, q + 1 in ONE pass; false = no such form for this M
    {
        if (v.rowmap)
            return launch_adc_list_prefilter2(qtab(q), prm(q), cand(j), ccnt(q), qtab(q + 1), prm(q + 1), cand(j + 1), ccnt(q + 1), p->M,
                                              codes(), v.rowmap, v.n, kCandCap, s);
        return launch_adc_prefilter2(qtab(q), prm(q), cand(j), ccnt(q), qtab(q + 1), prm(q + 1), cand(j + 1), ccnt(q + 1), p->M, codes(),
                                     v.n, kCandCap, s);
    }
    // The byte-table pass of the g = 4, 2 or 1 queries from `first`, as few walks over the codes as this M has forms for: four
    // queries share ONE pass (interleaved byte tables: one LDS gather per code byte serves all four; no such form over a
    // list), else two do, else each takes its own.
    void prefilter_group(int first, int g)
    {
        if (g == 4 && !v.rowmap) {
            const uint8_t *qt[4] = {qtab(first), qtab(first + 1), qtab(first + 2), qtab(first + 3)};
            const int *pr[4] = {prm(first), prm(first + 1), prm(first + 2), prm(first + 3)};
            uint32_t *cd[4] = {cand(0), cand(1), cand(2), cand(3)};
            uint32_t *cc[4] = {ccnt(first), ccnt(first + 1), ccnt(first + 2), ccnt(first + 3)};
            if (launch_adc_prefilter4(qt, pr, cd, cc, p->M, codes(), v.n, kCandCap, s)) { stats[1] += 4; return; }
        }
        int j = 0;
        for (; j + 1 < g; j += 2) {
            if (prefilter_two(first + j, j)) { stats[2] += 2; continue; }
            prefilter_one(first + j, j);
            prefilter_one(first + j + 1, j + 1);
            stats[3] += 2;
        }
        if (j < g) { prefilter_one(first + j, j); stats[3]++; }
    }
    // sampled threshold of one query: sample -> m-th best -> tau (cnt = 0)
    void threshold(int q)
    {
        if (v.rowmap) launch_adc_list_sample(tab(q), p->M, codes(), v.rowmap, v.n, plan.samp_count, sc.d_samp.get(), s);
        else launch_adc_sample(tab(q), p->M, codes(), v.n, plan.samp_count, sc.d_samp.get(), s);
        const uint32_t groups = launch_sample_topm(sc.d_samp.get(), plan.samp_count, plan.samp_m, sc.cs, q, s);
        if (!groups) throw std::logic_error("sample_plan"); // (never: see sample_plan; guard() answers LB_ERR_INTERNAL)
        launch_sample_tau(sc.cs, slot(q), 1, groups * (uint32_t)plan.samp_m, plan.samp_m, false, s); // sets tau, cnt = 0
    }
    // The sampled pass of the g queries from `first` (g > 1 only with the prefilter): the threshold of each, then ONE walk
    // over the codes.  With the prefilter, rows whose byte-table lower bound cannot pass tau are dropped and the survivors
    // are scored exactly.  params.ok == 0 (decided on the device: a table with NaN / negative / infinite entries): nothing is
    // admitted, the select flags the query (fewer than k entries) and the host redoes it on the exact schedule.
    void sampled_group(int first, int g)
    {
        for (int q = first; q < first + g; q++) {
            threshold(q);
            if (prefilter) launch_adc_quantise(tab(q), sc.d_minrng.get() + (size_t)q * p->M * 4, p->M, sc.cs.tau + q, qtab(q), prm(q), s);
        }
        const bool timed = prof && first + g == nq; // the pass that serves the last query
        if (timed) (void)hipEventRecord(sc.ev[2], s);
        if (prefilter) prefilter_group(first, g);
        else exact_scan(first, 0, v.n, false);
        if (timed) (void)hipEventRecord(sc.ev[3], s);
        const uint32_t k_have = (uint32_t)std::min<int64_t>(k, v.n);
        for (int j = 0; j < g; j++) {
            const int q = first + j;
            if (prefilter) launch_adc_exact_candidates(tab(q), p->M, codes(), cand(j), ccnt(q), kCandCap, prm(q), q, sc.cs, s);
            // the search's last select also writes the k results (redone queries overwrite them)
            launch_select(sc.cs, slot(q), 1, k, 0u, s, k_have, &em);
        }
    }
    // One query on the exact schedule: a bootstrap chunk, then chunks sized by what the list still holds (safe: chunks that
    // cannot overflow it).  What a search without a sampled plan runs, and what redoes a query the sampled pass missed.
    void chunked(int q, bool safe)
    {
        launch_init_cand(sc.cs, slot(q), 1, s);
        int64_t pos = 0;
        for (int step = 0; pos < v.n; step++) {
            const int64_t end = chunk_end_host(step, pos, v.n, k, plan.cap, safe, /*big_boot=*/true);
            const bool boot = step == 0;
            exact_scan(q, pos, end, boot);
            launch_select(sc.cs, slot(q), 1, k, boot ? (uint32_t)(end - pos) : 0u, s, 0u, end >= v.n ? &em : nullptr);
            pos = end;
        }
        if (v.n == 0) launch_emit_lists(sc.cs, slot(q), 1, k, nullptr, em.out_dist, em.out_labels, sc.h_flags.get(), s);
    }
    // Every query's first pass: quads while four queries remain, then a pair, then a single, where the queries of a group can
    // share a byte-table pass.  0, or the state of a fired context (the stream is drained then).
    int walk(const lb_cancel *ctx)
    {
        for (int q = 0, g; q < nq; q += g) {
            if (ctx && q > 0) { // a cancellable call waits for each pass before it enqueues the next (~10 us each)
                LB_HIP(hipStreamSynchronize(s));
                if (const int st = ctx_state(ctx)) return st;
            }
            const int left = nq - q;
            g = !prefilter ? 1 : left >= 4 && !v.rowmap ? 4 : left >= 2 ? 2 : 1;
            if (plan.samp_count) sampled_group(q, g);
            else chunked(q, false);
        }
        return 0;
    }
    int run(const float *d_queries, const lb_cancel *ctx)
    {
        if (prof) {
            for (auto &e : sc.ev)
                if (!e) LB_HIP(hipEventCreate(&e.h));
            LB_HIP(hipEventRecord(sc.ev[0], s));
        }
        launch_build_adc_table(p->d_codebooks.get(), p->M, p->K, p->sub, d_queries, nq, sc.d_tables.get(), s, prefilter ? sc.d_minrng.get() : nullptr,
                               sc.cs.flags, prefilter ? sc.d_cand_cnt.get() : nullptr); // (also clears the slots' status words)
        if (const int st = walk(ctx)) return ctx_fail(p, st);
        const uint32_t *flags = sc.h_flags.get(); // (each query's last select wrote its status word into the pinned h_flags)
        LB_HIP(hipStreamSynchronize(s));
        if (plan.samp_count) {
            bool any = false;
            for (int q = 0; q < nq; q++)
                if (flags[q] & (1u | 4u)) { chunked(q, false); stats[4]++; any = true; } // the sampled threshold missed
            if (any) LB_HIP(hipStreamSynchronize(s));
        }
        for (int q = 0; q < nq; q++)
            if (flags[q] & 1u) { chunked(q, true); stats[5]++; } // chunks that cannot overflow the list
        LB_LAUNCH_CHECK();
        if (prof) LB_HIP(hipEventRecord(sc.ev[1], s));
        LB_HIP(hipStreamSynchronize(s));
        float ms[2] = {0.f, 0.f};
        if (prof) {
            if (plan.samp_count && hipEventElapsedTime(&ms[0], sc.ev[2], sc.ev[3]) != hipSuccess) ms[0] = 0.f;
            if (hipEventElapsedTime(&ms[1], sc.ev[0], sc.ev[1]) != hipSuccess) ms[1] = 0.f;
            (void)hipGetLastError();
        }
        std::lock_guard<std::mutex> gs(p->stats_mu);
        std::copy(stats, stats + 6, p->last_stats);
        if (prof) std::copy(ms, ms + 2, p->prof_ms);
        return LB_OK;
    }
};

} // namespace

extern "C" {

lb_gpu_pq *lb_gpu_pq_new(int device, const uint8_t *blob, size_t len, int *out_status)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    if (!blob || len < 12) { st(LB_ERR_INVALID_ARG); return nullptr; } // "invalid PQ data: too short"
    const uint32_t dims = rd_u32le(blob), M = rd_u32le(blob + 4), K = rd_u32le(blob + 8);
    if (M == 0 || dims % M != 0) { st(LB_ERR_INVALID_ARG); return nullptr; } // "invalid PQ parameters"
    const size_t sub = dims / M;
    if (len != 12 + (size_t)M * K * sub * 4) { st(LB_ERR_INVALID_ARG); return nullptr; } // "size mismatch"
    if (K != 256) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    if ((size_t)M * 256 * 4 > 160 * 1024 - 1024) { st(LB_ERR_UNSUPPORTED); return nullptr; } // table must fit LDS
    return handle_open<lb_gpu_pq>(device, out_status, [&](lb_gpu_pq *p) {
        p->dims = (int)dims; p->M = (int)M; p->K = (int)K; p->sub = (int)sub;
        p->sc_free.reserve(4);
        p->d_codebooks.alloc((len - 12) / sizeof(float));
        // f32 little-endian on the wire == host/device layout on this platform
        LB_HIP(hipMemcpy(p->d_codebooks.get(), blob + 12, len - 12, hipMemcpyHostToDevice));
    });
}

void lb_gpu_pq_free(lb_gpu_pq *p) { handle_free(p); } // (the pooled scratch frees itself with the handle)
const char *lb_gpu_pq_last_error(const lb_gpu_pq *p) { return handle_last_error(p); }
int lb_gpu_pq_m(const lb_gpu_pq *p) { return p ? p->M : 0; }
int lb_gpu_pq_dims(const lb_gpu_pq *p) { return p ? p->dims : 0; }
int64_t lb_gpu_pq_ntotal(const lb_gpu_pq *p) { return handle_ntotal(p); }

// (not handle_reserve: that refuses 2^31 rows, a PQ handle holds up to 2^32 - 1)
int lb_gpu_pq_reserve(lb_gpu_pq *p, int64_t n_total)
{
    if (!p || n_total < 0) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(p->mu);
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        pq_grow(p, n_total);
        return LB_OK;
    });
}

int lb_gpu_pq_add_codes(lb_gpu_pq *p, int64_t n, const uint8_t *codes) { return add_codes_impl(p, n, codes, hipMemcpyHostToDevice); }
int lb_gpu_pq_add_codes_device(lb_gpu_pq *p, int64_t n, const uint8_t *d_codes) { return add_codes_impl(p, n, d_codes, hipMemcpyDeviceToDevice); }

// ---- the row filter (lb_handle.h) ---------------------------------------------------------------------------------------
int64_t lb_gpu_pq_nvisible(const lb_gpu_pq *p) { return filter_nvisible(p); }
int lb_gpu_pq_set_filter(lb_gpu_pq *p, const uint8_t *mask, int64_t n) { return filter_set(p, mask, n); }
int lb_gpu_pq_filter_int64(lb_gpu_pq *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                           int64_t validity_offset, int combine)
{
    return filter_column<int64_t>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_pq_filter_float32(lb_gpu_pq *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                             int64_t validity_offset, int combine)
{
    return filter_column<float>(p, column, n, value, op, validity, validity_offset, combine);
}

int lb_gpu_pq_get_codes(lb_gpu_pq *p, int64_t row0, int64_t n, uint8_t *codes)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        LB_HIP(hipMemcpy(codes, p->d_codes.get() + (size_t)row0 * p->M, (size_t)n * p->M, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- Encode / Decode -------------------------------------------------------------------
int lb_gpu_pq_encode_device(lb_gpu_pq *p, int64_t n, const float *d_vectors, uint8_t *d_codes, void *stream)
{
    if (!p || n < 0 || (n > 0 && (!d_vectors || !d_codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        launch_pq_encode(p->d_codebooks.get(), p->M, p->K, p->sub, d_vectors, n, d_codes, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

int lb_gpu_pq_encode(lb_gpu_pq *p, int64_t n, const float *vectors, uint8_t *codes)
{
    if (!p || n < 0 || (n > 0 && (!vectors || !codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    return host_codec(p, n, vectors, (size_t)p->dims * 4, codes, (size_t)p->M, [&](void *dv, void *dc, int64_t cnt) {
        return lb_gpu_pq_encode_device(p, cnt, static_cast<float *>(dv), static_cast<uint8_t *>(dc), nullptr);
    });
}

int lb_gpu_pq_add_vectors_device(lb_gpu_pq *p, int64_t n, const float *d_vectors)
{
    if (!p || n < 0 || (n > 0 && !d_vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    return pq_append(p, n, [&](uint8_t *dst) { launch_pq_encode(p->d_codebooks.get(), p->M, p->K, p->sub, d_vectors, n, dst, p->stream); });
}

int lb_gpu_pq_decode_device(lb_gpu_pq *p, int64_t n, const uint8_t *d_codes, float *d_vectors, void *stream)
{
    if (!p || n < 0 || (n > 0 && (!d_vectors || !d_codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        launch_pq_decode(p->d_codebooks.get(), p->M, p->K, p->sub, d_codes, n, d_vectors, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

int lb_gpu_pq_decode(lb_gpu_pq *p, int64_t n, const uint8_t *codes, float *vectors)
{
    if (!p || n < 0 || (n > 0 && (!vectors || !codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    return host_codec(p, n, codes, (size_t)p->M, vectors, (size_t)p->dims * 4, [&](void *dc, void *dv, int64_t cnt) {
        return lb_gpu_pq_decode_device(p, cnt, static_cast<uint8_t *>(dc), static_cast<float *>(dv), nullptr);
    });
}

// ---- ADC table / batch ----------------------------------------------------------------
int lb_gpu_pq_build_adc_table(lb_gpu_pq *p, const float *query, float *table)
{
    if (!p || !query || !table) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    Lease dq, dt;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        dq.reset(p->device, (size_t)p->dims * 4);
        dt.reset(p->device, (size_t)p->M * p->K * 4);
        LB_HIP(hipMemcpyAsync(dq.p, query, (size_t)p->dims * 4, hipMemcpyHostToDevice, p->stream));
        launch_build_adc_table(p->d_codebooks.get(), p->M, p->K, p->sub, dq.as<float>(), 1, dt.as<float>(), p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpyAsync(table, dt.p, (size_t)p->M * p->K * 4, hipMemcpyDeviceToHost, p->stream));
        LB_HIP(hipStreamSynchronize(p->stream));
        return LB_OK;
    });
}

int lb_gpu_pq_adc_distance_batch(lb_gpu_pq *p, const float *table, int64_t row0, int64_t n, float *results)
{
    if (!p || n < 0 || row0 < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK; // adc_table.go:58-60
    if (!table || !results) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (row0 + n > p->n) { p->set_error("flatCodes buffer too small"); return LB_ERR_INVALID_ARG; } // adc_table.go:61-63
    Lease dt, dr;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        dt.reset(p->device, (size_t)p->M * 256 * 4);
        dr.reset(p->device, (size_t)n * 4);
        LB_HIP(hipMemcpyAsync(dt.p, table, (size_t)p->M * 256 * 4, hipMemcpyHostToDevice, p->stream));
        CandState cs{};
        launch_adc_scan(dt.as<float>(), p->M, p->d_codes.get(), row0, row0 + n, 0, nullptr, cs, false, dr.as<float>(), row0,
                        p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpyAsync(results, dr.p, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
        LB_HIP(hipStreamSynchronize(p->stream));
        return LB_OK;
    });
}

// ---- candidate re-rank (processChunkInternal, PQ branch) ----------------------------------
int lb_gpu_pq_rerank_device(lb_gpu_pq *p, const float *d_query, const int64_t *d_rows, int64_t n, float *d_dist,
                            float *d_score, void *stream)
{
    if (!p || n < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!d_query || !d_rows || !d_dist) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    Lease dt;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        dt.reset(p->device, (size_t)p->M * 256 * 4);
        launch_build_adc_table(p->d_codebooks.get(), p->M, p->K, p->sub, d_query, 1, dt.as<float>(), s);
        launch_adc_rerank(dt.as<float>(), p->M, p->d_codes.get(), p->n, d_rows, n, d_dist, d_score, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

int lb_gpu_pq_rerank(lb_gpu_pq *p, const float *query, const int64_t *rows, int64_t n, float *dist, float *score)
{
    if (!p || n < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!query || !rows || !dist) return LB_ERR_INVALID_ARG;
    Lease dq, drw, dd, ds;
    return guard(p, p->stream, [&]() -> int { // (the device call below runs on p->stream)
        LB_HIP(hipSetDevice(p->device));
        dq.reset(p->device, (size_t)p->dims * 4);
        drw.reset(p->device, (size_t)n * 8);
        dd.reset(p->device, (size_t)n * 4);
        ds.reset(p->device, (size_t)n * 4);
        LB_HIP(hipMemcpy(dq.p, query, (size_t)p->dims * 4, hipMemcpyHostToDevice));
        LB_HIP(hipMemcpy(drw.p, rows, (size_t)n * 8, hipMemcpyHostToDevice));
        const int rc = lb_gpu_pq_rerank_device(p, dq.as<float>(), drw.as<int64_t>(), n, dd.as<float>(), ds.as<float>(), nullptr);
        if (rc != LB_OK) return rc;
        LB_HIP(hipMemcpy(dist, dd.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (score) LB_HIP(hipMemcpy(score, ds.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

int lb_gpu_pq_set_profiling(lb_gpu_pq *p, int enable)
{
    if (!p) return LB_ERR_INVALID_ARG;
    p->profiling.store(enable ? 1 : 0);
    return LB_OK;
}

int lb_gpu_pq_last_timing(const lb_gpu_pq *p, float ms[2])
{
    if (!p || !ms) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->stats_mu);
    std::copy(p->prof_ms, p->prof_ms + 2, ms);
    return LB_OK;
}

// ---- search ----------------------------------------------------------------------------
int lb_gpu_pq_set_prefilter(lb_gpu_pq *p, int enable)
{
    if (!p) return LB_ERR_INVALID_ARG;
    p->prefilter.store(enable ? 1 : 0);
    return LB_OK;
}

int lb_gpu_pq_search_device_ctx(lb_gpu_pq *p, int64_t nq, const float *d_queries, int k, float *d_dist,
                                int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    const int rc = pq_knn_args(p, nq, d_queries, k, d_dist, d_labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    ScratchLoan loan{p, nullptr};
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        const RowView v = p->filter.view(p->n);
        // decided once, before the first launch: whether the queries take the sampled threshold and, with it, the prefilter
        const SamplePlan plan = sample_plan(v.n, k, std::max<uint32_t>(8192u, 4u * next_pow2_host((uint32_t)k)));
        loan.sc = acquire_scratch(p, (int)nq, plan.cap, plan.samp_count);
        PqSearch a{p, v, *loan.sc, s, (int)nq, k, plan, plan.samp_count != 0 && p->prefilter.load() != 0, p->profiling.load() != 0,
                   EmitArgs{k, nullptr, d_dist, d_labels, loan.sc->h_flags.get()}, {plan.samp_count ? nq : 0, 0, 0, 0, 0, 0}};
        return a.run(d_queries, ctx);
    });
}

int lb_gpu_pq_last_search_stats(const lb_gpu_pq *p, int64_t out[6])
{
    if (!p || !out) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->stats_mu);
    std::copy(p->last_stats, p->last_stats + 6, out);
    return LB_OK;
}

int lb_gpu_pq_search_device(lb_gpu_pq *p, int64_t nq, const float *d_queries, int k, float *d_dist,
                            int64_t *d_labels, void *stream)
{
    return lb_gpu_pq_search_device_ctx(p, nq, d_queries, k, d_dist, d_labels, stream, nullptr);
}

int lb_gpu_pq_search(lb_gpu_pq *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels)
{
    return lb_gpu_pq_search_ctx(p, nq, queries, k, dist, labels, nullptr);
}

// Host-pointer search of one or several requests with the same k as ONE device batch (two queries share a pass over the
// codes): borrowed host buffers -> pooled pinned slab -> HBM, results back through the slab -- small ones (the latency path)
// written into it by the last kernel itself.  The caller has answered k and the queries of each request; a combined batch
// holds at most SearchCombiner::kBatch of them.
static int pq_host_search_multi(lb_gpu_pq *p, HostReq *const *reqs, int nreq, int k, const lb_cancel *ctx)
{
    int64_t nq = 0;
    for (int i = 0; i < nreq; i++) nq += reqs[i]->nq;
    const HostSlab sl(nq, (size_t)p->dims * 4, k);
    Lease hs, dq;
    return guard(p, p->stream, [&]() -> int { // (the device search below runs on p->stream)
        LB_HIP(hipSetDevice(p->device));
        hs.reset(p->device, sl.total, /*pinned=*/true);
        dq.reset(p->device, sl.direct ? sl.qb : sl.total);
        char *hb = hs.as<char>(), *dbuf = dq.as<char>();
        sl.gather(reqs, nreq, hb);
        LB_HIP(hipMemcpy(dbuf, hb, sl.qb, hipMemcpyHostToDevice));
        char *obuf = sl.direct ? hb : dbuf;
        const int rc = lb_gpu_pq_search_device_ctx(p, nq, reinterpret_cast<const float *>(dbuf), k, reinterpret_cast<float *>(obuf + sl.doff),
                                                   reinterpret_cast<int64_t *>(obuf + sl.loff), nullptr, ctx);
        if (rc != LB_OK) return rc;
        if (!sl.direct) LB_HIP(hipMemcpy(hb + sl.doff, dbuf + sl.doff, sl.db + sl.lb, hipMemcpyDeviceToHost));
        sl.scatter(reqs, nreq, hb, k);
        return LB_OK;
    });
}

int lb_gpu_pq_search_ctx(lb_gpu_pq *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels,
                         const lb_cancel *ctx)
{
    // (without the context: as before, a host call answers it after k and nq, in the device search)
    const int rc = pq_knn_args(p, nq, queries, k, dist, labels, nullptr);
    if (rc != LB_OK || nq == 0) return rc;
    HostReq me{queries, nq, dist, labels, k};
    // (concurrent calls of a few queries each are answered together: two queries share a pass over the codes, 1.48x the
    // queries per second of one call after the other; a call with a cancellation context is searched on its own)
    if (!ctx && nq <= SearchCombiner::kMaxNq && p->combiner.on.load() != 0)
        return p->combiner.search(me, [p](HostReq *const *reqs, int n, int kk) { return pq_host_search_multi(p, reqs, n, kk, nullptr); });
    HostReq *one = &me;
    return pq_host_search_multi(p, &one, 1, k, ctx);
}

int lb_gpu_pq_set_search_combining(lb_gpu_pq *p, int enable) { return combining_set(p, enable); }
int lb_gpu_pq_combining_stats(const lb_gpu_pq *p, int64_t out[2]) { return combining_stats(p, out); }

} // extern "C"
