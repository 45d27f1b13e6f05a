// ivfpq.hip -- host side of the lb_gpu_ivfpq_* entry points of include/longbow_gpu.h: the IVF-PQ index, the coarse partition of
// the IVF-Flat handle (ivf.hip) over the codes of the PQ handle (pq.hip).  The new kernels are in kernels_ivfpq.hip; the coarse
// quantiser is an inner exact f32 index over the centroids, the lists are kernels_ivf.hip's, the codec and the table
// kernels_pq.hip's and kernels_pq2.hip's.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_handle.h"
#include "lb_ivfpq.h"

#include <atomic>
#include <functional>
#include <vector>

using namespace lb;

struct lb_gpu_ivfpq : CodeHandle { // searches and reads share mu; adds and reserve take it alone
    int M = 0, K = 0, sub = 0, order = 0, nlist = 0;
    lb_gpu_index *coarse = nullptr; // the centroids: same device and dims, L2, the handle's order
    std::vector<float> h_cent;      // [nlist][dims]
    DevBuf<float> d_codebooks;      // [M][K][sub]
    DevBuf<uint8_t> d_codes;        // [capacity][M], insertion order: what get_codes returns
    DevBuf<int64_t> d_ids;          // [capacity] when ids were given
    bool has_ids = false;
    DevBuf<uint32_t> d_assign;      // [capacity]: list of each row
    // the lists and the list-major codes are built for all rows by every add, into the pair that is not in use: a failed add
    // leaves the old ones
    DevBuf<uint32_t> d_off[2];      // [nlist + 1]
    DevBuf<uint32_t> d_list[2];     // [capacity]
    DevBuf<uint8_t> d_lcodes[2];    // [capacity][M]: lcodes[pos] = codes[list[pos]]
    int cur = 0;
    std::vector<int64_t> h_sizes;   // [nlist]: sizes grids and scratch without a device round trip
    int64_t stats[4] = {0, 0, 0, 0}; // of the last search (under err_mu)
    std::atomic<bool> profiling{false};
    float timing[5] = {0, 0, 0, 0, 0}; // of the last profiled search (under err_mu): probes, plan, tables, scan, select; ms summed over its batches
    ~lb_gpu_ivfpq() { lb_gpu_index_free(coarse); }
    IvfLists lists(int i) const { return IvfLists{d_off[i].get(), d_list[i].get(), nlist}; }
};

namespace {

constexpr int64_t kQueryBatch = 1024;              // queries per batch at most
constexpr int64_t kKeyScratch = (int64_t)1 << 30;  // bytes of keys a batch may hold

uint32_t rd_u32le(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// All or nothing: every new buffer is allocated and filled before the first one replaces an old one.
void ivfpq_grow(lb_gpu_ivfpq *p, int64_t need, bool want_ids)
{
    const bool ids_missing = want_ids && p->d_ids.count() < (size_t)std::max<int64_t>(p->capacity, 1);
    if (need <= p->capacity && !ids_missing) return;
    const int64_t cap = need <= p->capacity ? p->capacity : grow_capacity(p->capacity, need, (size_t)p->M);
    DevBuf<int64_t> ni;
    if (want_ids) {
        ni.alloc((size_t)cap);
        if (p->n > 0 && p->has_ids) LB_HIP(hipMemcpy(ni.get(), p->d_ids.get(), (size_t)p->n * 8, hipMemcpyDeviceToDevice));
    }
    if (cap != p->capacity) {
        DevBuf<uint8_t> nc, nlc[2];
        DevBuf<uint32_t> na, nl[2];
        nc.alloc((size_t)cap * p->M);
        na.alloc((size_t)cap);
        for (int i = 0; i < 2; i++) {
            nl[i].alloc((size_t)cap);
            nlc[i].alloc((size_t)cap * p->M);
        }
        if (p->n > 0) {
            LB_HIP(hipMemcpy(nc.get(), p->d_codes.get(), (size_t)p->n * p->M, hipMemcpyDeviceToDevice));
            LB_HIP(hipMemcpy(na.get(), p->d_assign.get(), (size_t)p->n * 4, hipMemcpyDeviceToDevice));
            LB_HIP(hipMemcpy(nl[p->cur].get(), p->d_list[p->cur].get(), (size_t)p->n * 4, hipMemcpyDeviceToDevice));
            LB_HIP(hipMemcpy(nlc[p->cur].get(), p->d_lcodes[p->cur].get(), (size_t)p->n * p->M, hipMemcpyDeviceToDevice));
        }
        p->d_codes = std::move(nc);
        p->d_assign = std::move(na);
        for (int i = 0; i < 2; i++) {
            p->d_list[i] = std::move(nl[i]);
            p->d_lcodes[i] = std::move(nlc[i]);
        }
        p->capacity = cap;
    }
    if (want_ids) p->d_ids = std::move(ni);
}

// the coarse index's own refusal becomes the handle's; what the call enqueued on s is drained before its pooled buffers go back
int coarse_fail(lb_gpu_ivfpq *p, int rc, hipStream_t s)
{
    (void)hipStreamSynchronize(s);
    if (rc == LB_ERR_CANCELLED || rc == LB_ERR_DEADLINE) return ctx_fail(p, rc);
    p->set_error("coarse quantiser: %s", lb_gpu_last_error(p->coarse));
    return rc;
}

// The vectors are assigned and encoded in pieces of piece_rows(dims) rows (64 Mi floats: 256 MB of host vectors staged at a time,
// 12 bytes of labels and distances a row of a piece) and are not kept.  Codes and lists of the new rows are written behind the
// stored ones, where they belong to nobody until the commit.
int add_impl(lb_gpu_ivfpq *p, int64_t n, const float *vectors, const int64_t *ids, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (p->n > 0 && (ids != nullptr) != p->has_ids) {
        p->set_error("ids are given on every add or on none: the handle's rows have %s", p->has_ids ? "ids" : "none");
        return LB_ERR_INVALID_ARG;
    }
    if (const int st = rows_fit(p, p->n, n)) return st;
    Lease vec, lab, hist;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        const int64_t total = p->n + n;
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        std::vector<uint32_t> h_off((size_t)p->nlist + 1);
        std::vector<int64_t> sizes((size_t)p->nlist);
        ivfpq_grow(p, total, ids != nullptr);
        if (ids) LB_HIP(hipMemcpyAsync(p->d_ids.get() + p->n, ids, (size_t)n * 8, kind, s));
        // 1. the vectors, a piece at a time: 2. their lists (the k = 1 search of each over the centroids, narrowed), 3. their codes
        const int64_t piece = std::min(n, piece_rows(p->dims));
        const size_t lb = up16((size_t)piece * 8);
        lab.reset(p->device, lb + (size_t)piece * 4);
        int64_t *d_lab = lab.as<int64_t>();
        float *d_dist = reinterpret_cast<float *>(lab.as<char>() + lb);
        if (!on_device) vec.reset(p->device, (size_t)piece * p->dims * 4);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            const float *d_new = vectors + (size_t)r0 * p->dims;
            if (!on_device) {
                LB_HIP(hipMemcpyAsync(vec.p, d_new, (size_t)cnt * p->dims * 4, hipMemcpyHostToDevice, s));
                d_new = vec.as<float>();
            }
            if (const int rc = lb_gpu_index_search_device(p->coarse, cnt, d_new, 1, d_dist, d_lab, s)) return coarse_fail(p, rc, s);
            launch_ivf_narrow(d_lab, cnt, p->d_assign.get() + p->n + r0, s);
            launch_pq_encode(p->d_codebooks.get(), p->M, p->K, p->sub, d_new, cnt, p->d_codes.get() + (size_t)(p->n + r0) * p->M, s);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(s)); // (the staging buffer and the labels are reused by the next piece)
        }
        // 4. the lists of all rows and 5. their codes in list order, into the pair not in use
        const int nxt = 1 - p->cur;
        hist.reset(p->device, ivf_sort_hist_words(total, p->nlist) * 4);
        LB_HIP(launch_ivf_sort(p->d_assign.get(), total, p->nlist, hist.as<uint32_t>(), p->d_off[nxt].get(), p->d_list[nxt].get(), s));
        launch_ivfpq_permute(p->d_codes.get(), p->d_list[nxt].get(), total, p->M, p->d_lcodes[nxt].get(), s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpyAsync(h_off.data(), p->d_off[nxt].get(), h_off.size() * 4, hipMemcpyDeviceToHost, s));
        LB_HIP(hipStreamSynchronize(s));
        if ((int64_t)h_off[p->nlist] != total) {
            p->set_error("the lists hold %lld of %lld rows", (long long)h_off[p->nlist], (long long)total);
            return LB_ERR_INTERNAL;
        }
        for (int l = 0; l < p->nlist; l++) sizes[l] = (int64_t)h_off[l + 1] - (int64_t)h_off[l];
        // 6. commit (nothing below throws)
        p->h_sizes.swap(sizes);
        p->cur = nxt;
        p->has_ids = ids != nullptr;
        p->n = total;
        return LB_OK;
    });
}

// Exact ADC k-NN of nq device-resident queries among the rows of their probed lists; the caller holds the reader lock, has made
// the device current and has checked the arguments.  ctx is polled before every launch.  The scratch is leased into the caller's
// `sc`, declared outside the caller's guard as lb_handle.h asks of every pooled buffer.
int ivfpq_search_dev(lb_gpu_ivfpq *p, int64_t nq, const float *d_Q, int k, int nprobe, float *d_dist, int64_t *d_labels, hipStream_t s,
                     const lb_cancel *ctx, Lease &sc)
{
    int64_t st[4] = {nq, 0, 0, 0};
    auto publish = [&]() {
        std::lock_guard<std::mutex> g(p->err_mu);
        std::copy(st, st + 4, p->stats);
    };
    if (p->n == 0) { // all padding, without a launch
        LB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_dist), 0x7f7fffff /* FLT_MAX */, (size_t)nq * k, s));
        LB_HIP(hipMemsetAsync(d_labels, 0xff, (size_t)nq * k * 8, s));
        LB_HIP(hipStreamSynchronize(s));
        publish();
        return LB_OK;
    }
    const int np = std::min(nprobe, p->nlist);
    // pmax: the rows a query can scan at most, the sum of the np largest lists
    std::vector<int64_t> big(p->h_sizes);
    std::partial_sort(big.begin(), big.begin() + np, big.end(), std::greater<int64_t>());
    int64_t pmax = 0;
    for (int i = 0; i < np; i++) pmax += big[i];
    pmax = std::max<int64_t>(pmax, 1);
    const int64_t nb = std::min(std::min(nq, kQueryBatch), std::max<int64_t>(1, kKeyScratch / 8 / pmax));
    IvfBatch a{};
    a.X = nullptr; // (only the plan and the selection take the batch as the IVF-Flat kernels do: neither reads rows)
    a.D = p->dims;
    a.L = p->lists(p->cur);
    a.np = np;
    a.pmax = pmax;
    const uint8_t *lcodes = p->d_lcodes[p->cur].get();
    int64_t *d_probes = nullptr;
    float *d_pdist = nullptr, *d_tables = nullptr;
    unsigned long long *d_stats = nullptr;
    auto layout = [&](Carve c) {
        a.probes = d_probes = c.take<int64_t>((size_t)nb * np * 8);
        d_pdist = c.take<float>((size_t)nb * np * 4);
        a.seg = c.take<uint32_t>((size_t)nb * (np + 1) * 4);
        d_stats = c.take<unsigned long long>(4 * 8);
        d_tables = c.take<float>((size_t)nb * p->M * 256 * 4);
        a.keys = c.take<uint64_t>((size_t)nb * pmax * 8);
        return c.off;
    };
    lease_layout(sc, p->device, layout);
    int cancelled = 0;
    auto go = [&]() { // false: the context fired, nothing more is enqueued
        cancelled = ctx_state(ctx);
        return cancelled == 0;
    };
    if (go()) LB_HIP(hipMemsetAsync(d_stats, 0, 4 * 8, s));
    // profiling: events between the steps, read after each batch (tools/ivfpq_bench.py); it costs a drain per batch
    const bool prof = p->profiling.load();
    EventH ev[6];
    float tms[5] = {0, 0, 0, 0, 0};
    if (prof)
        for (EventH &e : ev) LB_HIP(hipEventCreate(&e.h));
    auto mark = [&](int i) { if (prof) LB_HIP(hipEventRecord(ev[i], s)); };
    for (int64_t q0 = 0; q0 < nq && !cancelled; q0 += nb) {
        a.nq = (int)std::min(nb, nq - q0);
        a.Q = d_Q + (size_t)q0 * p->dims;
        mark(0);
        // 1. the probes (the inner index polls ctx before its own launches).  More than LB_MAX_K of them is more than the coarse
        //    search returns: with every list probed they are all the lists, and their order does not reach the result
        if (np == p->nlist && np > LB_MAX_K) launch_ivf_all_probes(d_probes, a.nq, np, s);
        else if (const int rc = lb_gpu_index_search_device_ctx(p->coarse, a.nq, a.Q, np, d_pdist, d_probes, s, ctx)) return coarse_fail(p, rc, s);
        mark(1);
        if (!go()) break;
        launch_ivf_plan(a, d_stats, s);                                                                      // 2.
        mark(2);
        if (!go()) break;
        launch_build_adc_table(p->d_codebooks.get(), p->M, p->K, p->sub, a.Q, a.nq, d_tables, s);            // 3.
        mark(3);
        if (!go()) break;
        launch_ivfpq_scan(a, d_tables, p->M, lcodes, p->n, s);                                               // 4.
        mark(4);
        if (!go()) break;
        launch_ivf_select(a, k, p->has_ids ? p->d_ids.get() : nullptr, d_dist + (size_t)q0 * k, d_labels + (size_t)q0 * k, s); // 5.
        mark(5);
        if (prof) {
            LB_HIP(hipEventSynchronize(ev[5]));
            for (int i = 0; i < 5; i++) {
                float ms = 0.f;
                LB_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
                tms[i] += ms;
            }
        }
    }
    LB_LAUNCH_CHECK();
    unsigned long long h_stats[4] = {0, 0, 0, 0};
    if (!cancelled) LB_HIP(hipMemcpyAsync(h_stats, d_stats, sizeof h_stats, hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    if (cancelled) return ctx_fail(p, cancelled);
    for (int i = 1; i < 4; i++) st[i] = (int64_t)h_stats[i];
    publish();
    if (prof) {
        std::lock_guard<std::mutex> g(p->err_mu);
        std::copy(tms, tms + 5, p->timing);
    }
    return LB_OK;
}

int search_args(lb_gpu_ivfpq *p, int64_t nq, const void *queries, int k, int nprobe, const void *dist, const void *labels, const lb_cancel *ctx)
{
    return knn_args(p, nq, queries, k, dist, labels, ctx, [&]() -> int {
        if (nprobe <= 0) {
            p->set_error("nprobe=%d: at least one list is probed", nprobe);
            return LB_ERR_INVALID_ARG;
        }
        if (nprobe < p->nlist && nprobe > LB_MAX_K) {
            p->set_error("nprobe=%d: fewer than all %d lists are at most %d probes", nprobe, p->nlist, LB_MAX_K);
            return LB_ERR_UNSUPPORTED;
        }
        return LB_OK;
    });
}

} // namespace

extern "C" {

lb_gpu_ivfpq *lb_gpu_ivfpq_new(int device, const uint8_t *blob, size_t len, int order, int nlist, const float *centroids, int *out_status)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    // the blob, as lb_gpu_pq_new reads it (DeserializePQEncoder, internal/pq/persistence.go:38-73)
    if (!blob || len < 12 || order < 0 || order > 1 || nlist <= 0 || !centroids) { st(LB_ERR_INVALID_ARG); return nullptr; }
    const uint32_t dims = rd_u32le(blob), M = rd_u32le(blob + 4), K = rd_u32le(blob + 8);
    if (M == 0 || dims % M != 0) { st(LB_ERR_INVALID_ARG); return nullptr; }
    const size_t sub = dims / M;
    if (len != 12 + (size_t)M * K * sub * 4) { st(LB_ERR_INVALID_ARG); return nullptr; }
    if (K != 256 || (size_t)M * 256 * 4 > 160 * 1024 - 1024 || dims > LB_MAX_DIM || nlist > IVF_MAX_NLIST) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    int inner = LB_OK;
    lb_gpu_ivfpq *h = handle_open<lb_gpu_ivfpq>(device, out_status, [&](lb_gpu_ivfpq *p) {
        p->dims = (int)dims;
        p->M = (int)M;
        p->K = (int)K;
        p->sub = (int)sub;
        p->order = order;
        p->nlist = nlist;
        p->h_cent.assign(centroids, centroids + (size_t)nlist * dims);
        p->h_sizes.assign((size_t)nlist, 0);
        p->d_codebooks.alloc((len - 12) / sizeof(float));
        LB_HIP(hipMemcpy(p->d_codebooks.get(), blob + 12, len - 12, hipMemcpyHostToDevice)); // (f32 little-endian on the wire, as pq.hip)
        for (int i = 0; i < 2; i++) {
            p->d_off[i].alloc((size_t)nlist + 1);
            LB_HIP(hipMemset(p->d_off[i].get(), 0, ((size_t)nlist + 1) * 4));
        }
        p->coarse = lb_gpu_index_new(device, (int)dims, 0 /* L2 */, &inner);
        if (!p->coarse) return;
        inner = lb_gpu_index_set_order(p->coarse, order);
        if (inner == LB_OK) inner = lb_gpu_index_add(p->coarse, nlist, centroids, nullptr);
        LB_HIP(hipSetDevice(device));
    });
    if (h && inner != LB_OK) { // the centroids did not get onto the device
        handle_free(h);
        st(inner);
        return nullptr;
    }
    return h;
}

void lb_gpu_ivfpq_free(lb_gpu_ivfpq *p) { handle_free(p); }
const char *lb_gpu_ivfpq_last_error(const lb_gpu_ivfpq *p) { return handle_last_error(p); }
int lb_gpu_ivfpq_dims(const lb_gpu_ivfpq *p) { return p ? p->dims : 0; }
int lb_gpu_ivfpq_m(const lb_gpu_ivfpq *p) { return p ? p->M : 0; }
int lb_gpu_ivfpq_order(const lb_gpu_ivfpq *p) { return p ? p->order : 0; }
int lb_gpu_ivfpq_nlist(const lb_gpu_ivfpq *p) { return p ? p->nlist : 0; }
int64_t lb_gpu_ivfpq_ntotal(const lb_gpu_ivfpq *p) { return handle_ntotal(p); }

int64_t lb_gpu_ivfpq_hbm_bytes(const lb_gpu_ivfpq *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_ivfpq *>(p)->mu);
    return (int64_t)(p->d_codes.count() + p->d_lcodes[0].count() + p->d_lcodes[1].count() + p->d_ids.count() * 8 +
                     (p->d_assign.count() + p->d_list[0].count() + p->d_list[1].count() + p->d_off[0].count() + p->d_off[1].count()) * 4 +
                     p->d_codebooks.count() * 4) + lb_gpu_index_hbm_bytes(p->coarse);
}

int lb_gpu_ivfpq_get_centroids(lb_gpu_ivfpq *p, float *out)
{
    if (!p || !out) return LB_ERR_INVALID_ARG;
    std::copy(p->h_cent.begin(), p->h_cent.end(), out); // (fixed at creation)
    return LB_OK;
}

int lb_gpu_ivfpq_reserve(lb_gpu_ivfpq *p, int64_t n_total)
{
    return handle_reserve(p, n_total, [](lb_gpu_ivfpq *h, int64_t need) { ivfpq_grow(h, need, h->has_ids); });
}

int lb_gpu_ivfpq_add(lb_gpu_ivfpq *p, int64_t n, const float *vectors, const int64_t *ids) { return add_impl(p, n, vectors, ids, false); }
int lb_gpu_ivfpq_add_device(lb_gpu_ivfpq *p, int64_t n, const float *d_vectors, const int64_t *d_ids) { return add_impl(p, n, d_vectors, d_ids, true); }

int lb_gpu_ivfpq_get_codes(lb_gpu_ivfpq *p, int64_t row0, int64_t n, uint8_t *codes)
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

int lb_gpu_ivfpq_list_sizes(lb_gpu_ivfpq *p, int64_t *sizes)
{
    if (!p || !sizes) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    std::copy(p->h_sizes.begin(), p->h_sizes.end(), sizes);
    return LB_OK;
}

int lb_gpu_ivfpq_assignments(lb_gpu_ivfpq *p, int64_t row0, int64_t n, int32_t *lists)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !lists)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        LB_HIP(hipMemcpy(lists, p->d_assign.get() + row0, (size_t)n * 4, hipMemcpyDeviceToHost)); // (list numbers are below 2^16)
        return LB_OK;
    });
}

int lb_gpu_ivfpq_search_device_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels,
                                   void *stream, const lb_cancel *ctx)
{
    const int rc = search_args(p, nq, d_queries, k, nprobe, d_dist, d_labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    Lease sc;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        return ivfpq_search_dev(p, nq, d_queries, k, nprobe, d_dist, d_labels, s, ctx, sc);
    });
}

int lb_gpu_ivfpq_search_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                            const lb_cancel *ctx)
{
    const int rc = search_args(p, nq, queries, k, nprobe, dist, labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    return host_knn(
        p, nq, (size_t)p->dims * 4, k, dist, labels,
        [&](Lease &dq, Lease &, hipStream_t s) { LB_HIP(hipMemcpyAsync(dq.p, queries, (size_t)nq * p->dims * 4, hipMemcpyHostToDevice, s)); },
        [&](Lease &dq, float *d_dist, int64_t *d_labels, hipStream_t s, Lease &sc) {
            return ivfpq_search_dev(p, nq, dq.as<float>(), k, nprobe, d_dist, d_labels, s, ctx, sc);
        });
}

int lb_gpu_ivfpq_search(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels)
{
    return lb_gpu_ivfpq_search_ctx(p, nq, queries, k, nprobe, dist, labels, nullptr);
}

int lb_gpu_ivfpq_last_search_stats(lb_gpu_ivfpq *p, int64_t out[4])
{
    if (!p || !out) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->err_mu);
    std::copy(p->stats, p->stats + 4, out);
    return LB_OK;
}

int lb_gpu_ivfpq_set_profiling(lb_gpu_ivfpq *p, int enable)
{
    if (!p) return LB_ERR_INVALID_ARG;
    p->profiling.store(enable != 0);
    return LB_OK;
}

int lb_gpu_ivfpq_last_timing(lb_gpu_ivfpq *p, float ms[5])
{
    if (!p || !ms) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->err_mu);
    std::copy(p->timing, p->timing + 5, ms);
    return LB_OK;
}

} // extern "C"
