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
    // per-search scratch (lists, tables, sample and candidate buffers) is pooled on the handle: a search
    // must not hipMalloc/hipFree (the latter synchronises the device under every concurrent search)
    std::mutex sc_mu;
    std::vector<std::unique_ptr<PqScratch>> sc_free;
    // instrumentation (bench.py): HIP events around the main code pass and the whole search of the last query
    std::atomic<int> profiling{0};
    std::atomic<int> prefilter{1}; // 0 = exact f32-table pass only (lb_gpu_pq_set_prefilter; both are exact)
    SearchCombiner combiner;       // concurrent host-pointer searches of a few queries each are combined (lb_host.h)
    EventH ev[4];
    float prof_ms[2] = {0.f, 0.f};
    // what served the queries of the last COMPLETED device batch (lb_gpu_pq_last_search_stats): observing only
    mutable std::mutex stats_mu;
    int64_t last_stats[6] = {0, 0, 0, 0, 0, 0};
};

namespace {
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

constexpr uint32_t kCandCap = 65536; // prefilter survivors per query (expected: a few thousand)

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

void release_scratch(lb_gpu_pq *p, std::unique_ptr<PqScratch> sc)
{
    std::lock_guard<std::mutex> g(p->sc_mu);
    if (p->sc_free.size() < 4) p->sc_free.push_back(std::move(sc));
}

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

static int add_codes_impl(lb_gpu_pq *p, int64_t n, const uint8_t *codes, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (p->n + n > (int64_t)0xffffffffll) { p->set_error("more than 2^32 codes per device"); return LB_ERR_UNSUPPORTED; }
    if (p->filter.on)
        if (const int st = filter_fits(p, p->n + n)) return st;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        pq_grow(p, p->n + n);
        LB_HIP(hipMemcpy(p->d_codes.get() + (size_t)p->n * p->M, codes, (size_t)n * p->M,
                          on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        p->filter.on_append(p->n, p->n + n, p->stream);
        p->n += n;
        return LB_OK;
    });
}

int lb_gpu_pq_add_codes(lb_gpu_pq *p, int64_t n, const uint8_t *codes) { return add_codes_impl(p, n, codes, false); }
int lb_gpu_pq_add_codes_device(lb_gpu_pq *p, int64_t n, const uint8_t *d_codes) { return add_codes_impl(p, n, d_codes, true); }

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
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = stream ? (hipStream_t)stream : p->stream;
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
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (p->n + n > (int64_t)0xffffffffll) { p->set_error("more than 2^32 codes per device"); return LB_ERR_UNSUPPORTED; }
    if (p->filter.on)
        if (const int st = filter_fits(p, p->n + n)) return st;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        pq_grow(p, p->n + n);
        launch_pq_encode(p->d_codebooks.get(), p->M, p->K, p->sub, d_vectors, n, p->d_codes.get() + (size_t)p->n * p->M, p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(p->stream));
        p->filter.on_append(p->n, p->n + n, p->stream);
        p->n += n;
        return LB_OK;
    });
}

int lb_gpu_pq_decode_device(lb_gpu_pq *p, int64_t n, const uint8_t *d_codes, float *d_vectors, void *stream)
{
    if (!p || n < 0 || (n > 0 && (!d_vectors || !d_codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = stream ? (hipStream_t)stream : p->stream;
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
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        Lease dq(p->device, (size_t)p->dims * 4), dt(p->device, (size_t)p->M * p->K * 4);
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
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        Lease dt(p->device, (size_t)p->M * 256 * 4), dr(p->device, (size_t)n * 4);
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
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = stream ? (hipStream_t)stream : p->stream;
        Lease dt(p->device, (size_t)p->M * 256 * 4);
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
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        Lease dq(p->device, (size_t)p->dims * 4), drw(p->device, (size_t)n * 8), dd(p->device, (size_t)n * 4),
            ds(p->device, (size_t)n * 4);
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
    ms[0] = p->prof_ms[0];
    ms[1] = p->prof_ms[1];
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
    if (!p || nq < 0 || k <= 0 || (nq > 0 && (!d_queries || !d_dist || !d_labels))) return LB_ERR_INVALID_ARG;
    if (nq == 0) return LB_OK;
    if (const int st = ctx_state(ctx)) return ctx_fail(p, st);
    if (k > 4096) { p->set_error("k=%d exceeds the supported maximum 4096", k); return LB_ERR_UNSUPPORTED; }
    if (nq > 65536) { p->set_error("nq=%lld exceeds 65536 queries per call", (long long)nq); return LB_ERR_UNSUPPORTED; }
    std::shared_lock<std::shared_mutex> g(p->mu);
    std::unique_ptr<PqScratch> scp;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = stream ? (hipStream_t)stream : p->stream;
        const int nqi = (int)nq;
        // Under a row filter the search walks the v.n positions of the ascending list of visible rows (kernels_pq_list.hip)
        // instead of the p->n rows: the plan, the chunk schedule and the selects count positions, the entries carry rows.
        const RowView v = p->filter.view(p->n);
        const uint8_t *codes = p->d_codes.get();
        // Sampled admission threshold (same reasoning as index_search.hip: sample_plan): one row in `stride` is scored
        // exactly, the m-th best sample entry becomes tau, and the codes are walked once.  About m*stride rows
        // pass (4096 at stride 512); fewer than k or more than the list holds is detected by the select and
        // the query is redone by the bootstrap schedule.  Two-level m-th minimum: the sample (195k entries at
        // 100M rows) is larger than one list.  Stride 512 with a 16384-entry list (mean + 5 sigma = 11.3k
        // admitted rows) instead of stride 256 / 8192 halves the sampling pass (49 -> 25 us at 100M rows).
        uint32_t samp_count = 0;
        int samp_m = 0;
        uint32_t cap = std::max<uint32_t>(8192u, 4u * next_pow2_host((uint32_t)k));
        if (v.n >= 65536 && v.n < ((int64_t)1 << 32)) {
            const uint32_t cap_s = std::max<uint32_t>(16384u, cap);
            const int64_t stride = v.n >= ((int64_t)8192 * 512) ? 512 : 256;
            const int64_t cnt = std::max<int64_t>(8192, (v.n + stride - 1) / stride);
            const double lambda = (double)k * (double)cnt / (double)v.n;
            const int m = std::max(8, (int)std::ceil(lambda + 5.0 * std::sqrt(lambda) + 4.0));
            const double loose = (double)m * ((double)v.n / (double)cnt) * (1.0 + 5.0 / std::sqrt((double)m));
            if (m <= 32 && loose <= (double)(cap_s - (uint32_t)k) && cnt <= (int64_t)8192 * (8192 / m)) {
                samp_count = (uint32_t)cnt;
                samp_m = m;
                cap = cap_s;
            }
        }
        scp = acquire_scratch(p, nqi, cap, samp_count);
        PqScratch &sc = *scp;
        const bool prefilter = samp_count != 0 && p->prefilter.load() != 0;
        const bool prof = p->profiling.load() != 0;
        // {sampled plan, four-query pass, two-query pass, single prefilter pass, bootstrap redo, safe redo} (queries)
        int64_t stats[6] = {samp_count ? nqi : 0, 0, 0, 0, 0, 0};
        if (prof) {
            for (auto &e : p->ev)
                if (!e) LB_HIP(hipEventCreate(&e.h));
            LB_HIP(hipEventRecord(p->ev[0], s));
        }
        launch_build_adc_table(p->d_codebooks.get(), p->M, p->K, p->sub, d_queries, nqi, sc.d_tables.get(), s, prefilter ? sc.d_minrng.get() : nullptr,
                               sc.cs.flags, prefilter ? sc.d_cand_cnt.get() : nullptr); // (also clears the slots' status words)
        // the search's last select writes the k results AND the slot's status word into pinned host memory (no D2H copy)
        const EmitArgs em{k, nullptr, d_dist, d_labels, sc.h_flags.get()};
        const uint32_t k_have = (uint32_t)std::min<int64_t>(k, v.n);
        // the passes over the rows or, under a filter, over the list
        auto exact_scan = [&](const float *tab, int64_t begin, int64_t end, int q, bool boot) {
            if (v.rowmap) launch_adc_list_scan(tab, p->M, codes, v.rowmap, begin, end, q, sc.cs, boot, s);
            else launch_adc_scan(tab, p->M, codes, begin, end, q, nullptr, sc.cs, boot, nullptr, 0, s);
        };
        auto prefilter_one = [&](const uint8_t *qtab, const int *prm, uint32_t *cand, uint32_t *ccnt) {
            if (v.rowmap) launch_adc_list_prefilter(qtab, prm, p->M, codes, v.rowmap, v.n, cand, kCandCap, ccnt, s);
            else launch_adc_prefilter(qtab, prm, p->M, codes, v.n, cand, kCandCap, ccnt, s);
        };
        auto prefilter_two = [&](const uint8_t *qtab0, const int *prm0, uint32_t *cand0, uint32_t *ccnt0, const uint8_t *qtab1,
                                 const int *prm1, uint32_t *cand1, uint32_t *ccnt1) -> bool {
            if (v.rowmap)
                return launch_adc_list_prefilter2(qtab0, prm0, cand0, ccnt0, qtab1, prm1, cand1, ccnt1, p->M, codes, v.rowmap, v.n, kCandCap, s);
            return launch_adc_prefilter2(qtab0, prm0, cand0, ccnt0, qtab1, prm1, cand1, ccnt1, p->M, codes, v.n, kCandCap, s);
        };
        // sampled threshold of one query: sample -> m-th best -> tau (cnt = 0); false = no sampled pass for this search
        auto threshold = [&](int q) -> bool {
            const float *tab = sc.d_tables.get() + (size_t)q * p->M * 256;
            if (v.rowmap) launch_adc_list_sample(tab, p->M, codes, v.rowmap, v.n, samp_count, sc.d_samp.get(), s);
            else launch_adc_sample(tab, p->M, codes, v.n, samp_count, sc.d_samp.get(), s);
            const uint32_t groups = launch_sample_topm(sc.d_samp.get(), samp_count, samp_m, sc.cs, q, s);
            if (!groups) return false;
            launch_sample_tau(sc.cs, sc.d_slots.get() + q, 1, groups * (uint32_t)samp_m, samp_m, false, s); // sets tau, cnt = 0
            return true;
        };
        // mode 0: sampled threshold (+ byte-table prefilter), 1: bootstrap chunks, 2: chunks that cannot overflow
        auto scan_query = [&](int q, int mode) {
            const float *tab = sc.d_tables.get() + (size_t)q * p->M * 256;
            if (mode == 0 && samp_count) {
                if (threshold(q)) {
                    if (prefilter) {
                        // rows whose byte-table lower bound cannot pass tau are dropped; the survivors are scored
                        // exactly.  params.ok == 0 (decided on the device: a table with NaN / negative / infinite
                        // entries): nothing is admitted, the select below flags the query (fewer than k entries) and
                        // the host redoes it on the exact schedule.
                        int *prm = sc.d_params.get() + q * 4;
                        uint8_t *qtab = sc.d_qtabs.get() + (size_t)q * p->M * 256;
                        launch_adc_quantise(tab, sc.d_minrng.get() + (size_t)q * p->M * 4, p->M, sc.cs.tau + q, qtab, prm, s);
                        if (prof && q == nqi - 1) (void)hipEventRecord(p->ev[2], s);
                        prefilter_one(qtab, prm, sc.d_cand.get(), sc.d_cand_cnt.get() + q);
                        stats[3]++;
                        if (prof && q == nqi - 1) (void)hipEventRecord(p->ev[3], s);
                        launch_adc_exact_candidates(tab, p->M, p->d_codes.get(), sc.d_cand.get(), sc.d_cand_cnt.get() + q, kCandCap, prm, q,
                                                    sc.cs, s);
                    } else {
                        if (prof && q == nqi - 1) (void)hipEventRecord(p->ev[2], s);
                        exact_scan(tab, 0, v.n, q, false);
                        if (prof && q == nqi - 1) (void)hipEventRecord(p->ev[3], s);
                    }
                    // the search's last select also writes the k results (redone queries overwrite them below)
                    launch_select(sc.cs, sc.d_slots.get() + q, 1, k, 0u, s, k_have, &em);
                    return;
                }
            }
            launch_init_cand(sc.cs, sc.d_slots.get() + q, 1, s);
            int64_t pos = 0;
            int step = 0;
            while (pos < v.n) {
                const int64_t end = chunk_end_host(step, pos, v.n, k, cap, mode == 2, /*big_boot=*/true);
                const bool boot = step == 0;
                exact_scan(tab, pos, end, q, boot);
                launch_select(sc.cs, sc.d_slots.get() + q, 1, k, boot ? (uint32_t)(end - pos) : 0u, s, 0u,
                              end >= v.n ? &em : nullptr);
                pos = end;
                step++;
            }
            if (v.n == 0) launch_emit_lists(sc.cs, sc.d_slots.get() + q, 1, k, nullptr, d_dist, d_labels, sc.h_flags.get(), s);
        };
        // two queries share ONE pass over the codes: thresholds and byte tables for both, then the two-query
        // prefilter, then the exact survivors and the select of each.  false = not applicable (run them one by one)
        auto scan_pair = [&](int q) -> bool {
            if (!prefilter || !samp_count) return false;
            int *prm[2];
            uint8_t *qtab[2];
            for (int j = 0; j < 2; j++) {
                const int qq = q + j;
                const float *tab = sc.d_tables.get() + (size_t)qq * p->M * 256;
                if (!threshold(qq)) return false; // (never after the first of the pair succeeded: same counts)
                prm[j] = sc.d_params.get() + qq * 4;
                qtab[j] = sc.d_qtabs.get() + (size_t)qq * p->M * 256;
                launch_adc_quantise(tab, sc.d_minrng.get() + (size_t)qq * p->M * 4, p->M, sc.cs.tau + qq, qtab[j], prm[j], s);
            }
            const bool last = q + 1 == nqi - 1;
            if (prof && last) (void)hipEventRecord(p->ev[2], s);
            if (!prefilter_two(qtab[0], prm[0], sc.d_cand.get(), sc.d_cand_cnt.get() + q, qtab[1], prm[1], sc.d_cand.get() + kCandCap,
                               sc.d_cand_cnt.get() + q + 1)) {
                for (int j = 0; j < 2; j++)
                    prefilter_one(qtab[j], prm[j], sc.d_cand.get() + (size_t)j * kCandCap, sc.d_cand_cnt.get() + q + j);
                stats[3] += 2;
            } else {
                stats[2] += 2;
            }
            if (prof && last) (void)hipEventRecord(p->ev[3], s);
            for (int j = 0; j < 2; j++) {
                const int qq = q + j;
                const float *tab = sc.d_tables.get() + (size_t)qq * p->M * 256;
                launch_adc_exact_candidates(tab, p->M, p->d_codes.get(), sc.d_cand.get() + (size_t)j * kCandCap, sc.d_cand_cnt.get() + qq, kCandCap,
                                            prm[j], qq, sc.cs, s);
                launch_select(sc.cs, sc.d_slots.get() + qq, 1, k, 0u, s, k_have, &em);
            }
            return true;
        };
        // four queries share ONE pass (interleaved byte tables: one LDS gather per code byte serves all four)
        auto scan_quad = [&](int q) -> bool {
            if (!prefilter || !samp_count || v.rowmap) return false; // (no four-query form over a list: pairs serve it)
            const int *prm[4];
            const uint8_t *qtab[4];
            uint32_t *cand[4], *ccnt[4];
            for (int j = 0; j < 4; j++) {
                const int qq = q + j;
                const float *tab = sc.d_tables.get() + (size_t)qq * p->M * 256;
                if (!threshold(qq)) return false;
                int *prm_w = sc.d_params.get() + qq * 4;
                uint8_t *qt = sc.d_qtabs.get() + (size_t)qq * p->M * 256;
                launch_adc_quantise(tab, sc.d_minrng.get() + (size_t)qq * p->M * 4, p->M, sc.cs.tau + qq, qt, prm_w, s);
                prm[j] = prm_w; qtab[j] = qt;
                cand[j] = sc.d_cand.get() + (size_t)j * kCandCap;
                ccnt[j] = sc.d_cand_cnt.get() + qq;
            }
            const bool last = q + 3 == nqi - 1;
            if (prof && last) (void)hipEventRecord(p->ev[2], s);
            if (!launch_adc_prefilter4(qtab, prm, cand, ccnt, p->M, p->d_codes.get(), p->n, kCandCap, s)) {
                for (int j = 0; j < 4; j += 2)
                    if (!launch_adc_prefilter2(qtab[j], prm[j], cand[j], ccnt[j], qtab[j + 1], prm[j + 1], cand[j + 1], ccnt[j + 1], p->M,
                                               p->d_codes.get(), p->n, kCandCap, s)) {
                        for (int u = j; u < j + 2; u++)
                            launch_adc_prefilter(qtab[u], prm[u], p->M, p->d_codes.get(), p->n, cand[u], kCandCap, ccnt[u], s);
                        stats[3] += 2;
                    } else {
                        stats[2] += 2;
                    }
            } else {
                stats[1] += 4;
            }
            if (prof && last) (void)hipEventRecord(p->ev[3], s);
            for (int j = 0; j < 4; j++) {
                const int qq = q + j;
                const float *tab = sc.d_tables.get() + (size_t)qq * p->M * 256;
                launch_adc_exact_candidates(tab, p->M, p->d_codes.get(), cand[j], ccnt[j], kCandCap, prm[j], qq, sc.cs, s);
                launch_select(sc.cs, sc.d_slots.get() + qq, 1, k, 0u, s, k_have, &em);
            }
            return true;
        };
        for (int q = 0; q < nqi; q++) {
            if (ctx && q > 0) { // a cancellable call waits for each pass before it enqueues the next (~10 us each)
                LB_HIP(hipStreamSynchronize(s));
                if (const int st = ctx_state(ctx)) {
                    release_scratch(p, std::move(scp));
                    return ctx_fail(p, st);
                }
            }
            if (q + 3 < nqi && scan_quad(q)) {
                q += 3;
                continue;
            }
            if (q + 1 < nqi && scan_pair(q)) {
                q++;
                continue;
            }
            scan_query(q, 0);
        }
        auto read_flags = [&]() { // (each query's last select wrote its status word into the pinned h_flags)
            LB_HIP(hipStreamSynchronize(s));
        };
        read_flags();
        if (samp_count) {
            bool any = false;
            for (int q = 0; q < nqi; q++)
                if (sc.h_flags.get()[q] & (1u | 4u)) { scan_query(q, 1); stats[4]++; any = true; } // the sampled threshold missed
            if (any) read_flags();
        }
        for (int q = 0; q < nqi; q++)
            if (sc.h_flags.get()[q] & 1u) { scan_query(q, 2); stats[5]++; } // chunks that cannot overflow the list
        LB_LAUNCH_CHECK();
        if (prof) LB_HIP(hipEventRecord(p->ev[1], s));
        LB_HIP(hipStreamSynchronize(s));
        if (prof) {
            float a = 0.f, b = 0.f;
            if (samp_count && hipEventElapsedTime(&a, p->ev[2], p->ev[3]) != hipSuccess) a = 0.f;
            if (hipEventElapsedTime(&b, p->ev[0], p->ev[1]) != hipSuccess) b = 0.f;
            (void)hipGetLastError();
            p->prof_ms[0] = a;
            p->prof_ms[1] = b;
        }
        release_scratch(p, std::move(scp));
        {
            std::lock_guard<std::mutex> gs(p->stats_mu);
            std::copy(stats, stats + 6, p->last_stats);
        }
        return LB_OK;
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
// written into it by the last kernel itself.
static int pq_host_search_multi(lb_gpu_pq *p, HostReq *const *reqs, int nreq, int k, const lb_cancel *ctx)
{
    int64_t nq = 0;
    for (int i = 0; i < nreq; i++) nq += reqs[i]->nq;
    if (k > 4096) { p->set_error("k=%d exceeds the supported maximum 4096", k); return LB_ERR_UNSUPPORTED; }
    if (nq > 65536) { p->set_error("nq=%lld exceeds 65536 queries per call", (long long)nq); return LB_ERR_UNSUPPORTED; }
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        const size_t qb = (size_t)nq * p->dims * 4, db = up16((size_t)nq * k * 4), lbb = (size_t)nq * k * 8;
        const size_t doff = up16(qb), loff = doff + db, total = loff + lbb;
        const bool direct = db + lbb <= ((size_t)64 << 10);
        Lease hs(p->device, total, /*pinned=*/true), dq(p->device, direct ? qb : total);
        char *hb = hs.as<char>(), *dbuf = dq.as<char>();
        size_t off = 0;
        for (int i = 0; i < nreq; i++) {
            const size_t b = (size_t)reqs[i]->nq * p->dims * 4;
            std::memcpy(hb + off, reqs[i]->q, b);
            off += b;
        }
        LB_HIP(hipMemcpy(dbuf, hb, qb, hipMemcpyHostToDevice));
        char *obuf = direct ? hb : dbuf;
        const int rc = lb_gpu_pq_search_device_ctx(p, nq, reinterpret_cast<const float *>(dbuf), k, reinterpret_cast<float *>(obuf + doff),
                                                   reinterpret_cast<int64_t *>(obuf + loff), nullptr, ctx);
        if (rc != LB_OK) return rc;
        if (!direct) LB_HIP(hipMemcpy(hb + doff, dbuf + doff, db + lbb, hipMemcpyDeviceToHost));
        size_t row = 0;
        for (int i = 0; i < nreq; i++) {
            const size_t n = (size_t)reqs[i]->nq * k;
            std::memcpy(reqs[i]->dist, hb + doff + row * 4, n * 4);
            std::memcpy(reqs[i]->labels, hb + loff + row * 8, n * 8);
            row += n;
        }
        return LB_OK;
    });
}

int lb_gpu_pq_search_ctx(lb_gpu_pq *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels,
                         const lb_cancel *ctx)
{
    if (!p || nq < 0 || k <= 0 || (nq > 0 && (!queries || !dist || !labels))) return LB_ERR_INVALID_ARG;
    if (nq == 0) return LB_OK;
    HostReq me{queries, nq, dist, labels, k};
    // (concurrent calls of a few queries each are answered together: two queries share a pass over the codes, 1.48x the
    // queries per second of one call after the other; a call with a cancellation context is searched on its own)
    if (!ctx && nq <= SearchCombiner::kMaxNq && k <= 4096 && p->combiner.on.load() != 0)
        return p->combiner.search(me, [p](HostReq *const *reqs, int n, int kk) { return pq_host_search_multi(p, reqs, n, kk, nullptr); });
    HostReq *one = &me;
    return pq_host_search_multi(p, &one, 1, k, ctx);
}

int lb_gpu_pq_set_search_combining(lb_gpu_pq *p, int enable)
{
    if (!p) return LB_ERR_INVALID_ARG;
    p->combiner.on.store(enable ? 1 : 0);
    return LB_OK;
}

int lb_gpu_pq_combining_stats(const lb_gpu_pq *p, int64_t out[2])
{
    if (!p || !out) return LB_ERR_INVALID_ARG;
    out[0] = p->combiner.batches.load();
    out[1] = p->combiner.requests.load();
    return LB_OK;
}

} // extern "C"
