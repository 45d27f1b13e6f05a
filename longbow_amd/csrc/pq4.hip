// pq4.hip -- host side of the lb_gpu_pq4_* entry points of include/longbow_gpu.h: 16-centroid codebooks, 4-bit codes packed two
// to a byte in HBM (lb_pq4.h), exact ADC k-NN over them.
//
// Codebooks arrive as the reference's serialised blob with DeserializePQEncoder's validation, as in pq.hip; K must be 16.  The
// reference handles small K as a case of its own: Encode's K <= 16 branch (encodeSequential, internal/pq/encoder.go:87-120),
// BuildADCTable and ADCDistance at stride K (adc_table.go:46, 77-92).  The search follows the schedule of pq.hip's exact
// (non-prefilter) path -- boot chunks for a corpus that fits a list, otherwise sample, tau, one admission pass, select -- with
// up to four queries sharing each pass over the codes.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_handle.h"
#include "lb_pq4.h"

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
struct Pq4Scratch;
} // namespace

struct lb_gpu_pq4 : CodeHandle { // searches and reads share mu; adds and reserve take it alone
    int M = 0, sub = 0, P = 0;   // P: bytes of a packed row
    DevBuf<float> d_codebooks;
    DevBuf<uint8_t> d_codes;     // [capacity][P]
    DevBuf<uint32_t> d_bad;      // the packing kernel's offender flag
    PinnedBuf<uint32_t> h_bad;
    // per-search scratch is pooled on the handle, as on lb_gpu_pq: a search must not hipMalloc / hipFree
    std::mutex sc_mu;
    std::vector<std::unique_ptr<Pq4Scratch>> sc_free;
};

namespace {
constexpr int kPqMaxK = 4096;       // largest k of a search (the list of a query holds 4 * k entries)
constexpr int64_t kPqMaxNq = 65536; // queries per call

void pq4_grow(lb_gpu_pq4 *p, int64_t need)
{
    if (need <= p->capacity) return;
    const int64_t cap = grow_capacity(p->capacity, need, (size_t)p->P);
    DevBuf<uint8_t> nc;
    nc.alloc((size_t)cap * p->P);
    if (p->n > 0) LB_HIP(hipMemcpy(nc.get(), p->d_codes.get(), (size_t)p->n * p->P, hipMemcpyDeviceToDevice));
    p->d_codes = std::move(nc);
    p->capacity = cap;
}

// n more rows: fill(dst) enqueues on p->stream whatever writes their packed bytes at dst.  The offender flag is read before the
// rows are committed (p->n): a refused batch leaves the handle as it was.
template <class Fill> int pq4_append(lb_gpu_pq4 *p, int64_t n, Fill &&fill)
{
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (p->n + n > (int64_t)0xffffffffll) { p->set_error("more than 2^32 codes per device"); return LB_ERR_UNSUPPORTED; }
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        pq4_grow(p, p->n + n);
        LB_HIP(hipMemsetAsync(p->d_bad.get(), 0, sizeof(uint32_t), p->stream));
        fill(p->d_codes.get() + (size_t)p->n * p->P);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpyAsync(p->h_bad.get(), p->d_bad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
        LB_HIP(hipStreamSynchronize(p->stream));
        if (*p->h_bad.get()) { p->set_error("a code of 16 or more in a batch of 4-bit codes"); return LB_ERR_INVALID_ARG; }
        p->n += n;
        return LB_OK;
    });
}

// rows per staging piece of an add from host memory
int64_t pq4_piece(int64_t n, size_t row_bytes) { return std::min<int64_t>(n, std::max<int64_t>(1, ((int64_t)256 << 20) / (int64_t)row_bytes)); }

int add_codes_impl(lb_gpu_pq4 *p, int64_t n, const uint8_t *codes, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    Lease stage;
    return pq4_append(p, n, [&](uint8_t *dst) {
        if (on_device) { launch_pq4_pack(codes, p->M, n, dst, p->d_bad.get(), p->stream); return; }
        const int64_t piece = pq4_piece(n, (size_t)p->M);
        stage.reset(p->device, (size_t)piece * p->M);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            LB_HIP(hipMemcpyAsync(stage.p, codes + (size_t)r0 * p->M, (size_t)cnt * p->M, hipMemcpyHostToDevice, p->stream));
            launch_pq4_pack(stage.as<uint8_t>(), p->M, cnt, dst + (size_t)r0 * p->P, p->d_bad.get(), p->stream);
            if (r0 + piece < n) LB_HIP(hipStreamSynchronize(p->stream)); // (the stage is filled again)
        }
    });
}

int add_vectors_impl(lb_gpu_pq4 *p, int64_t n, const float *vectors, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    Lease stage;
    return pq4_append(p, n, [&](uint8_t *dst) {
        if (on_device) { launch_pq4_encode(p->d_codebooks.get(), p->M, p->sub, vectors, n, dst, true, p->stream); return; }
        const size_t row = (size_t)p->dims * 4;
        const int64_t piece = pq4_piece(n, row);
        stage.reset(p->device, (size_t)piece * row);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            LB_HIP(hipMemcpyAsync(stage.p, vectors + (size_t)r0 * p->dims, (size_t)cnt * row, hipMemcpyHostToDevice, p->stream));
            launch_pq4_encode(p->d_codebooks.get(), p->M, p->sub, stage.as<float>(), cnt, dst + (size_t)r0 * p->P, true, p->stream);
            if (r0 + piece < n) LB_HIP(hipStreamSynchronize(p->stream));
        }
    });
}

// What a k-NN entry point answers before it touches the device (pq.hip: pq_knn_args)
int pq4_knn_args(lb_gpu_pq4 *p, int64_t nq, const void *queries, int k, const void *dist, const void *labels, const lb_cancel *ctx)
{
    if (!p || nq < 0 || k <= 0 || (nq > 0 && (!queries || !dist || !labels))) return LB_ERR_INVALID_ARG;
    if (nq == 0) return LB_OK;
    if (const int st = ctx_state(ctx)) return ctx_fail(p, st);
    if (k > kPqMaxK) { p->set_error("k=%d exceeds the supported maximum %d", k, kPqMaxK); return LB_ERR_UNSUPPORTED; }
    if (nq > kPqMaxNq) { p->set_error("nq=%lld exceeds %lld queries per call", (long long)nq, (long long)kPqMaxNq); return LB_ERR_UNSUPPORTED; }
    return LB_OK;
}

struct Pq4Scratch {
    int device = 0;
    int nq_cap = 0;
    CandState cs{}; // pointers into the four buffers below
    DevBuf<uint64_t> d_lists, d_tau;
    DevBuf<uint32_t> d_cnt, d_flags;
    DevBuf<float> d_tables;  // [nq][M * 16]
    DevBuf<int> d_slots;     // 0 .. nq - 1
    DevBuf<uint64_t> d_samp; // entries of the sampled rows
    PinnedBuf<uint32_t> h_flags;
    ~Pq4Scratch() { (void)hipSetDevice(device); }
};

std::unique_ptr<Pq4Scratch> acquire_scratch(lb_gpu_pq4 *p, int nq, uint32_t cap, size_t samp_entries)
{
    std::unique_ptr<Pq4Scratch> sc;
    {
        std::lock_guard<std::mutex> g(p->sc_mu);
        for (size_t i = 0; i < p->sc_free.size(); i++)
            if (p->sc_free[i]->nq_cap >= nq && p->sc_free[i]->cs.cap == cap) {
                sc = std::move(p->sc_free[i]);
                p->sc_free.erase(p->sc_free.begin() + (long)i);
                break;
            }
    }
    if (!sc) {
        sc = std::make_unique<Pq4Scratch>();
        sc->device = p->device;
        sc->nq_cap = std::max(nq, 4);
        const size_t nqc = (size_t)sc->nq_cap;
        sc->d_lists.alloc(nqc * cap);
        sc->d_cnt.alloc(nqc);
        sc->d_tau.alloc(nqc);
        sc->d_flags.alloc(nqc);
        sc->cs.lists = sc->d_lists.get();
        sc->cs.cnt = sc->d_cnt.get();
        sc->cs.tau = sc->d_tau.get();
        sc->cs.flags = sc->d_flags.get();
        sc->cs.cap = cap;
        sc->d_tables.alloc(nqc * p->M * PQ4_K);
        sc->d_slots.alloc(nqc);
        sc->h_flags.alloc(nqc);
        std::vector<int> slots(nqc);
        for (size_t q = 0; q < nqc; q++) slots[q] = (int)q;
        LB_HIP(hipMemcpy(sc->d_slots.get(), slots.data(), nqc * sizeof(int), hipMemcpyHostToDevice));
    }
    sc->d_samp.ensure(samp_entries);
    return sc;
}

// A search's hold on its scratch (pq.hip: ScratchLoan): back to the pool on every path, once the stream is drained
struct Pq4Loan {
    lb_gpu_pq4 *p;
    std::unique_ptr<Pq4Scratch> sc;
    ~Pq4Loan()
    {
        std::lock_guard<std::mutex> g(p->sc_mu);
        if (sc && p->sc_free.size() < 4) p->sc_free.push_back(std::move(sc)); // (lb_gpu_pq4_new reserved the room: nothing throws)
    }
};

// One device batch.  The chunk schedule and the plan depend on n and k alone, so the queries of a group walk the same row
// ranges: a group of g queries takes ONE pass over the codes for each step, then a select per query.
struct Pq4Search {
    lb_gpu_pq4 *p;
    Pq4Scratch &sc;
    hipStream_t s;
    int nq, k;
    AdcSamplePlan plan;
    bool lds; // tables in LDS below PQ4_REG_MAX_M too (pq4_lds_lookup)
    const lb_cancel *ctx;
    EmitArgs em; // the search's last select writes the k results and the slot's status word into pinned host memory

    const float *tab(int q) const { return sc.d_tables.get() + (size_t)q * p->M * PQ4_K; }
    const int *slot(int q) const { return sc.d_slots.get() + q; }
    void poll() const { ctx_check(ctx); } // before every launch; guard() drains the stream and answers the context's state

    void scan(int first, int g, int64_t begin, int64_t end, bool boot)
    {
        poll();
        launch_pq4_scan(tab(first), p->M, p->d_codes.get(), begin, end, first, g, sc.cs, boot, nullptr, 0, lds, s);
    }
    // sampled threshold of one query: sample -> m-th best -> tau (cnt = 0)
    void threshold(int q)
    {
        poll();
        launch_pq4_sample(tab(q), p->M, p->d_codes.get(), p->n, plan.samp_count, sc.d_samp.get(), lds, s);
        poll();
        const uint32_t groups = launch_sample_topm(sc.d_samp.get(), plan.samp_count, plan.samp_m, sc.cs, q, s);
        if (!groups) throw std::logic_error("adc_sample_plan"); // (never: see adc_sample_plan; guard() answers LB_ERR_INTERNAL)
        poll();
        launch_sample_tau(sc.cs, slot(q), 1, groups * (uint32_t)plan.samp_m, plan.samp_m, false, s);
    }
    void sampled_group(int first, int g)
    {
        for (int q = first; q < first + g; q++) threshold(q);
        scan(first, g, 0, p->n, false);
        const uint32_t k_have = (uint32_t)std::min<int64_t>(k, p->n);
        for (int q = first; q < first + g; q++) {
            poll();
            launch_select(sc.cs, slot(q), 1, k, 0u, s, k_have, &em);
        }
    }
    // The exact schedule: a bootstrap chunk, then chunks sized by what the list still holds (safe: chunks that cannot overflow
    // it).  What a search without a sampled plan runs, and what redoes a query whose list overflowed or stayed short.
    void chunked(int first, int g, bool safe)
    {
        for (int q = first; q < first + g; q++) { poll(); launch_init_cand(sc.cs, slot(q), 1, s); }
        int64_t pos = 0;
        for (int step = 0; pos < p->n; step++) {
            const int64_t end = chunk_end_host(step, pos, p->n, k, plan.cap, safe, /*big_boot=*/true);
            const bool boot = step == 0;
            scan(first, g, pos, end, boot);
            for (int q = first; q < first + g; q++) {
                poll();
                launch_select(sc.cs, slot(q), 1, k, boot ? (uint32_t)(end - pos) : 0u, s, 0u, end >= p->n ? &em : nullptr);
            }
            pos = end;
        }
        if (p->n == 0)
            for (int q = first; q < first + g; q++) {
                poll();
                launch_emit_lists(sc.cs, slot(q), 1, k, nullptr, em.out_dist, em.out_labels, sc.h_flags.get(), s);
            }
    }
    int run(const float *d_queries)
    {
        poll();
        launch_build_adc_table(p->d_codebooks.get(), p->M, PQ4_K, p->sub, d_queries, nq, sc.d_tables.get(), s, nullptr, sc.cs.flags, nullptr);
        const int gmax = pq4_max_queries_per_pass(p->M, lds);
        for (int q = 0, g; q < nq; q += g) {
            const int left = nq - q;
            g = left >= 4 && gmax >= 4 ? 4 : left >= 2 ? 2 : 1;
            if (plan.samp_count) sampled_group(q, g);
            else chunked(q, g, false);
        }
        const uint32_t *flags = sc.h_flags.get(); // (each query's last select wrote its status word)
        LB_HIP(hipStreamSynchronize(s));
        if (plan.samp_count) {
            bool any = false;
            for (int q = 0; q < nq; q++)
                if (flags[q] & (1u | 4u)) { chunked(q, 1, false); any = true; } // the sampled threshold missed
            if (any) LB_HIP(hipStreamSynchronize(s));
        }
        for (int q = 0; q < nq; q++)
            if (flags[q] & 1u) chunked(q, 1, true); // chunks that cannot overflow the list
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    }
};

// Which lookup serves M <= PQ4_REG_MAX_M.  Measured at 1M rows, M = 96: the staged scan with the tables in LDS takes
// 17.9 us a query (two a pass), with the tables in registers 19.8 us (four a pass), so rows that take the fast form are looked
// up in LDS; the generic form keeps the register lookup.  LB_PQ4_LOOKUP (diagnostic build): 0 registers, 1 LDS.
bool pq4_lds_lookup(const lb_gpu_pq4 *p)
{
    const int t = lb_tunable("LB_PQ4_LOOKUP", -1);
    return t >= 0 ? t != 0 : p->P % 16 == 0;
}

} // namespace

extern "C" {

lb_gpu_pq4 *lb_gpu_pq4_new(int device, const uint8_t *blob, size_t len, int *out_status)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    if (!blob || len < 12) { st(LB_ERR_INVALID_ARG); return nullptr; } // "invalid PQ data: too short"
    const uint32_t dims = rd_u32le(blob), M = rd_u32le(blob + 4), K = rd_u32le(blob + 8);
    if (M == 0 || dims % M != 0) { st(LB_ERR_INVALID_ARG); return nullptr; } // "invalid PQ parameters"
    const size_t sub = dims / M;
    if (len != 12 + (size_t)M * K * sub * 4) { st(LB_ERR_INVALID_ARG); return nullptr; } // "size mismatch"
    if (K != (uint32_t)PQ4_K || M > (uint32_t)PQ4_MAX_M || dims > (uint32_t)LB_MAX_DIM) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    return handle_open<lb_gpu_pq4>(device, out_status, [&](lb_gpu_pq4 *p) {
        p->dims = (int)dims; p->M = (int)M; p->sub = (int)sub; p->P = pq4_row_bytes((int)M);
        p->sc_free.reserve(4);
        p->d_bad.alloc(1);
        p->h_bad.alloc(1);
        p->d_codebooks.alloc((len - 12) / sizeof(float));
        // f32 little-endian on the wire == host/device layout on this platform
        LB_HIP(hipMemcpy(p->d_codebooks.get(), blob + 12, len - 12, hipMemcpyHostToDevice));
    });
}

void lb_gpu_pq4_free(lb_gpu_pq4 *p) { handle_free(p); }
const char *lb_gpu_pq4_last_error(const lb_gpu_pq4 *p) { return handle_last_error(p); }
int lb_gpu_pq4_m(const lb_gpu_pq4 *p) { return p ? p->M : 0; }
int lb_gpu_pq4_dims(const lb_gpu_pq4 *p) { return p ? p->dims : 0; }
int64_t lb_gpu_pq4_ntotal(const lb_gpu_pq4 *p) { return handle_ntotal(p); }

int64_t lb_gpu_pq4_hbm_bytes(const lb_gpu_pq4 *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_pq4 *>(p)->mu);
    return p->capacity * (int64_t)p->P + (int64_t)p->M * PQ4_K * p->sub * 4;
}

// (not handle_reserve: that refuses 2^31 rows, this handle holds up to 2^32 - 1)
int lb_gpu_pq4_reserve(lb_gpu_pq4 *p, int64_t n_total)
{
    if (!p || n_total < 0) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (n_total > (int64_t)0xffffffffll) { p->set_error("more than 2^32 codes per device"); return LB_ERR_UNSUPPORTED; }
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        pq4_grow(p, n_total);
        return LB_OK;
    });
}

int lb_gpu_pq4_add_codes(lb_gpu_pq4 *p, int64_t n, const uint8_t *codes) { return add_codes_impl(p, n, codes, false); }
int lb_gpu_pq4_add_codes_device(lb_gpu_pq4 *p, int64_t n, const uint8_t *d_codes) { return add_codes_impl(p, n, d_codes, true); }
int lb_gpu_pq4_add_vectors(lb_gpu_pq4 *p, int64_t n, const float *vectors) { return add_vectors_impl(p, n, vectors, false); }
int lb_gpu_pq4_add_vectors_device(lb_gpu_pq4 *p, int64_t n, const float *d_vectors) { return add_vectors_impl(p, n, d_vectors, true); }

int lb_gpu_pq4_get_codes(lb_gpu_pq4 *p, int64_t row0, int64_t n, uint8_t *codes)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    Lease out;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        const int64_t piece = pq4_piece(n, (size_t)p->M);
        out.reset(p->device, (size_t)piece * p->M);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            launch_pq4_unpack(p->d_codes.get() + (size_t)(row0 + r0) * p->P, p->M, cnt, out.as<uint8_t>(), p->stream);
            LB_LAUNCH_CHECK();
            LB_HIP(hipMemcpyAsync(codes + (size_t)r0 * p->M, out.p, (size_t)cnt * p->M, hipMemcpyDeviceToHost, p->stream));
            LB_HIP(hipStreamSynchronize(p->stream));
        }
        return LB_OK;
    });
}

int lb_gpu_pq4_encode_device(lb_gpu_pq4 *p, int64_t n, const float *d_vectors, uint8_t *d_codes, void *stream)
{
    if (!p || n < 0 || (n > 0 && (!d_vectors || !d_codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        launch_pq4_encode(p->d_codebooks.get(), p->M, p->sub, d_vectors, n, d_codes, false, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

int lb_gpu_pq4_encode(lb_gpu_pq4 *p, int64_t n, const float *vectors, uint8_t *codes)
{
    if (!p || n < 0 || (n > 0 && (!vectors || !codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    return host_codec(p, n, vectors, (size_t)p->dims * 4, codes, (size_t)p->M, [&](void *dv, void *dc, int64_t cnt) {
        return lb_gpu_pq4_encode_device(p, cnt, static_cast<float *>(dv), static_cast<uint8_t *>(dc), nullptr);
    });
}

int lb_gpu_pq4_build_adc_table(lb_gpu_pq4 *p, const float *query, float *table)
{
    if (!p || !query || !table) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    Lease dq, dt;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        const size_t tb = (size_t)p->M * PQ4_K * 4;
        dq.reset(p->device, (size_t)p->dims * 4);
        dt.reset(p->device, tb);
        LB_HIP(hipMemcpyAsync(dq.p, query, (size_t)p->dims * 4, hipMemcpyHostToDevice, p->stream));
        launch_build_adc_table(p->d_codebooks.get(), p->M, PQ4_K, p->sub, dq.as<float>(), 1, dt.as<float>(), p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpyAsync(table, dt.p, tb, hipMemcpyDeviceToHost, p->stream));
        LB_HIP(hipStreamSynchronize(p->stream));
        return LB_OK;
    });
}

int lb_gpu_pq4_adc_distance_batch(lb_gpu_pq4 *p, const float *table, int64_t row0, int64_t n, float *results)
{
    if (!p || n < 0 || row0 < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK; // adc_table.go:58-60
    if (!table || !results) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    Lease dt, dr;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        const size_t tb = (size_t)p->M * PQ4_K * 4;
        dt.reset(p->device, tb);
        dr.reset(p->device, (size_t)n * 4);
        LB_HIP(hipMemcpyAsync(dt.p, table, tb, hipMemcpyHostToDevice, p->stream));
        launch_pq4_scan(dt.as<float>(), p->M, p->d_codes.get(), row0, row0 + n, 0, 1, CandState{}, false, dr.as<float>(), row0,
                        pq4_lds_lookup(p), p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpyAsync(results, dr.p, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
        LB_HIP(hipStreamSynchronize(p->stream));
        return LB_OK;
    });
}

int lb_gpu_pq4_search_device_ctx(lb_gpu_pq4 *p, int64_t nq, const float *d_queries, int k, float *d_dist, int64_t *d_labels,
                                 void *stream, const lb_cancel *ctx)
{
    const int rc = pq4_knn_args(p, nq, d_queries, k, d_dist, d_labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    Pq4Loan loan{p, nullptr};
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        // decided once, before the first launch: whether the queries take the sampled threshold
        const AdcSamplePlan plan = adc_sample_plan(p->n, k, std::max<uint32_t>(8192u, 4u * next_pow2_host((uint32_t)k)));
        loan.sc = acquire_scratch(p, (int)nq, plan.cap, plan.samp_count);
        Pq4Search a{p, *loan.sc, s, (int)nq, k, plan, pq4_lds_lookup(p), ctx, EmitArgs{k, nullptr, d_dist, d_labels, loan.sc->h_flags.get()}};
        return a.run(d_queries);
    });
}

// Host-pointer search: borrowed host buffers -> pooled pinned slab -> HBM, results back through the slab -- small ones written
// into it by the last kernel itself (pq.hip: pq_host_search_multi, for one request)
int lb_gpu_pq4_search_ctx(lb_gpu_pq4 *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    const int rc = pq4_knn_args(p, nq, queries, k, dist, labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    HostReq me{queries, nq, dist, labels, k};
    HostReq *one = &me;
    const HostSlab sl(nq, (size_t)p->dims * 4, k);
    Lease hs, dq;
    return guard(p, p->stream, [&]() -> int { // (the device search below runs on p->stream)
        LB_HIP(hipSetDevice(p->device));
        hs.reset(p->device, sl.total, /*pinned=*/true);
        dq.reset(p->device, sl.direct ? sl.qb : sl.total);
        char *hb = hs.as<char>(), *dbuf = dq.as<char>();
        sl.gather(&one, 1, hb);
        LB_HIP(hipMemcpy(dbuf, hb, sl.qb, hipMemcpyHostToDevice));
        char *obuf = sl.direct ? hb : dbuf;
        const int rc2 = lb_gpu_pq4_search_device_ctx(p, nq, reinterpret_cast<const float *>(dbuf), k, reinterpret_cast<float *>(obuf + sl.doff),
                                                     reinterpret_cast<int64_t *>(obuf + sl.loff), nullptr, ctx);
        if (rc2 != LB_OK) return rc2;
        if (!sl.direct) LB_HIP(hipMemcpy(hb + sl.doff, dbuf + sl.doff, sl.db + sl.lb, hipMemcpyDeviceToHost));
        sl.scatter(&one, 1, hb, k);
        return LB_OK;
    });
}

int lb_gpu_pq4_search(lb_gpu_pq4 *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels)
{
    return lb_gpu_pq4_search_ctx(p, nq, queries, k, dist, labels, nullptr);
}

} // extern "C"
