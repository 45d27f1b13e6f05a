// ivfbq.hip -- host side of the lb_gpu_ivfbq_* entry points of include/longbow_gpu.h: the IVF-BQ index, the coarse partition of
// the IVF-Flat handle (ivf.hip) over the codes of the BQ handle (bq.hip).  The new kernels are in kernels_ivfbq.hip; the coarse
// quantiser is an inner exact f32 index over the centroids, the lists are kernels_ivf.hip's, the codec kernels_bq.hip's, the
// list-major copy kernels_ivfpq.hip's and the selection kernels_ivfsq8.hip's.  The codes are list-major, as on the IVF-PQ handle,
// so under a row filter the visible lists hold positions.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_ivf_host.h"
#include "lb_ivfbq.h"
#include "lb_ivfpq.h"
#include "lb_ivfsq8.h"

using namespace lb;

struct lb_gpu_ivfbq : IvfHandle { // the partition (L2), and under a row filter the visible lists of positions (lb_ivf_host.h)
    int order = 0, W = 0;
    DevBuf<uint64_t> d_codes;       // [capacity][W], insertion order: what get_codes returns
    // the list-major codes are built for all rows by every add, with the lists, into the pair that is not in use
    DevBuf<uint64_t> d_lcodes[2];   // [capacity][W]: lcodes[pos] = codes[list[pos]]
    float timing[5] = {0, 0, 0, 0, 0}; // of the last profiled search (under err_mu): probes, plan, the queries' codes, scan, select; ms summed over its batches
    size_t row_words(int64_t rows) const { return (size_t)rows * (size_t)W; }
};

namespace {

// All or nothing: every new buffer is allocated and filled before the first one replaces an old one.
void ivfbq_grow(lb_gpu_ivfbq *p, int64_t need, bool want_ids)
{
    const int64_t cap = ivf_grow_to(p, p->part, need, want_ids, (size_t)p->W * 8); // 1.
    if (cap < 0) return;
    IvfGrowth g;                                                                    // 2.
    DevBuf<uint64_t> nc, nlc[2];
    const int cur = p->part.cur;
    g.stage(p, cap, want_ids);
    if (g.resize) {
        nc.alloc(p->row_words(cap));
        for (DevBuf<uint64_t> &l : nlc) l.alloc(p->row_words(cap));
        if (p->n > 0) {
            LB_HIP(hipMemcpy(nc.get(), p->d_codes.get(), p->row_words(p->n) * 8, hipMemcpyDeviceToDevice));
            LB_HIP(hipMemcpy(nlc[cur].get(), p->d_lcodes[cur].get(), p->row_words(p->n) * 8, hipMemcpyDeviceToDevice));
        }
        p->filter.grow(p->n, cap);                                                  // 3. (the last step that can fail)
    }
    g.commit(p);                                                                    // 4.
    if (!g.resize) return;
    p->d_codes = std::move(nc);
    for (int i = 0; i < 2; i++) p->d_lcodes[i] = std::move(nlc[i]);
    p->capacity = cap;
}

// The vectors are assigned and encoded in pieces of piece_rows(dims) rows (64 Mi floats: 256 MB of host vectors staged at a time,
// 12 bytes of labels and distances a row of a piece) and are not kept.  Codes and lists of the new rows are written behind the
// stored ones, where they belong to nobody until the commit.
int add_impl(lb_gpu_ivfbq *p, int64_t n, const float *vectors, const int64_t *ids, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    IvfPartition &P = p->part;
    if (const int st = ivf_ids_consistent(p, P, ids)) return st;
    if (const int st = rows_fit(p, p->n, n)) return st;
    Lease vec, lab, hist, vis;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        const int64_t total = p->n + n;
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        std::vector<int64_t> sizes, vsizes;
        const bool filtered = p->filter.on;
        ivfbq_grow(p, total, ids != nullptr);
        if (ids) LB_HIP(hipMemcpyAsync(P.d_ids.get() + p->n, ids, (size_t)n * 8, kind, s));
        // 1. the vectors, a piece at a time: 2. their lists, 3. their codes
        const int64_t piece = std::min(n, piece_rows(p->dims));
        lab.reset(p->device, ivf_assign_bytes(piece));
        if (!on_device) vec.reset(p->device, (size_t)piece * p->dims * 4);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            const float *d_new = vectors + (size_t)r0 * p->dims;
            if (!on_device) {
                LB_HIP(hipMemcpyAsync(vec.p, d_new, (size_t)cnt * p->dims * 4, hipMemcpyHostToDevice, s));
                d_new = vec.as<float>();
            }
            if (const int rc = ivf_assign(p, P, p->n + r0, cnt, d_new, lab, s)) return rc;
            launch_bq_encode(d_new, cnt, p->dims, p->d_codes.get() + p->row_words(p->n + r0), s);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(s)); // (the staging buffer and the labels are reused by the next piece)
        }
        // 4. the lists of all rows and 5. their codes in list order, into the pair not in use
        const int nxt = 1 - P.cur;
        ivf_sort_lists(p, P, total, hist, s);
        launch_ivfpq_permute(reinterpret_cast<const uint8_t *>(p->d_codes.get()), P.d_list[nxt].get(), total, 8 * p->W,
                             reinterpret_cast<uint8_t *>(p->d_lcodes[nxt].get()), s);
        if (const int rc = ivf_read_lists(p, P, total, sizes, s)) return rc;
        // 6. under a filter the new rows are visible: the visible lists of all rows, from the new lists (every position changes
        //    with them), into the pair not in use
        const int64_t nvis = filtered ? ivf_add_visible(p, total, vis, vsizes, s) : 0;
        // 7. commit (nothing below throws)
        if (filtered) ivf_commit_visible(p, vsizes, nvis);
        P.h_sizes.swap(sizes);
        P.cur = nxt;
        P.has_ids = ids != nullptr;
        p->n = total;
        return LB_OK;
    });
}

// The handle's call of the search loop (lb_ivf_host.h): exact Hamming k-NN; under a filter it walks the visible lists.  Its middle
// steps are the queries' codes, a timing slot of their own, and the scan of the list-major codes; the selection is the one over
// integer keys.
int ivfbq_search_dev(lb_gpu_ivfbq *p, int64_t nq, const float *d_Q, int k, int nprobe, float *d_dist, int64_t *d_labels, hipStream_t s,
                     const lb_cancel *ctx, Lease &sc)
{
    const IvfPartition &P = p->part;
    IvfBatch a{};
    a.X = nullptr; // (the plan and the selection take the batch as the IVF-Flat kernels do: neither reads rows)
    a.D = p->dims;
    const uint64_t *lcodes = p->d_lcodes[P.cur].get();
    const uint32_t *rows = P.d_list[P.cur].get();
    uint64_t *d_qc = nullptr;
    return ivf_search(
        p, p->part, p->lists(), p->sizes(), a, nq, d_Q, k, nprobe, d_dist, d_labels, s, ctx, sc, p->timing, 5,
        [&](Carve &c, IvfBatch &, int64_t nb) { d_qc = c.take<uint64_t>(p->row_words(nb) * 8); },
        [&](const IvfBatch &b, int64_t maxlen, auto &&, auto &&next) {
            if (!next()) return false; // (the plan's slot ends here)
            launch_bq_encode(b.Q, b.nq, p->dims, d_qc, s);
            if (!next()) return false;
            const IvfBqScan scan{b, lcodes, rows, p->n, p->W, d_qc, p->filter.on ? p->filter.n_visible : 0};
            if (p->filter.on) launch_ivfbq_scan_visible(scan, maxlen, s);
            else launch_ivfbq_scan(scan, maxlen, s);
            return true;
        },
        kQueryBatch, launch_ivfsq8_select);
}

} // namespace

extern "C" {

lb_gpu_ivfbq *lb_gpu_ivfbq_new(int device, int dims, int order, int nlist, const float *centroids, int *out_status)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    if (dims <= 0 || !centroids || order < 0 || order > 1 || nlist <= 0) { st(LB_ERR_INVALID_ARG); return nullptr; }
    if (dims > LB_MAX_DIM || nlist > IVF_MAX_NLIST) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    return ivf_open<lb_gpu_ivfbq>(device, dims, 0 /* L2 */, order, nlist, centroids, out_status, [&](lb_gpu_ivfbq *p) {
        p->order = order;
        p->W = (dims + 63) / 64;
        p->positions = true; // a visible list addresses the list-major codes
    });
}

void lb_gpu_ivfbq_free(lb_gpu_ivfbq *p) { handle_free(p); }
const char *lb_gpu_ivfbq_last_error(const lb_gpu_ivfbq *p) { return handle_last_error(p); }
int lb_gpu_ivfbq_dims(const lb_gpu_ivfbq *p) { return p ? p->dims : 0; }
int lb_gpu_ivfbq_words(const lb_gpu_ivfbq *p) { return p ? p->W : 0; }
int lb_gpu_ivfbq_order(const lb_gpu_ivfbq *p) { return p ? p->order : 0; }
int lb_gpu_ivfbq_nlist(const lb_gpu_ivfbq *p) { return p ? p->part.nlist : 0; }
int64_t lb_gpu_ivfbq_ntotal(const lb_gpu_ivfbq *p) { return handle_ntotal(p); }

int64_t lb_gpu_ivfbq_hbm_bytes(const lb_gpu_ivfbq *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_ivfbq *>(p)->mu);
    return (int64_t)((p->d_codes.count() + p->d_lcodes[0].count() + p->d_lcodes[1].count()) * 8) + p->visible_bytes() + p->part.hbm_bytes();
}

int lb_gpu_ivfbq_reserve(lb_gpu_ivfbq *p, int64_t n_total)
{
    return handle_reserve(p, n_total, [](lb_gpu_ivfbq *h, int64_t need) { ivfbq_grow(h, need, h->part.has_ids); });
}

int lb_gpu_ivfbq_get_codes(lb_gpu_ivfbq *p, int64_t row0, int64_t n, uint64_t *codes)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        LB_HIP(hipMemcpy(codes, p->d_codes.get() + p->row_words(row0), p->row_words(n) * 8, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- the row filter (lb_handle.h, lb_ivf_host.h) ------------------------------------------------------------------------
int64_t lb_gpu_ivfbq_nvisible(const lb_gpu_ivfbq *p) { return filter_nvisible(p); }
int lb_gpu_ivfbq_set_filter(lb_gpu_ivfbq *p, const uint8_t *mask, int64_t n) { return ivf_set_filter(p, mask, n); }
int lb_gpu_ivfbq_filter_int64(lb_gpu_ivfbq *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                              int64_t validity_offset, int combine)
{
    return ivf_filter_column<int64_t>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivfbq_filter_float32(lb_gpu_ivfbq *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                                int64_t validity_offset, int combine)
{
    return ivf_filter_column<float>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivfbq_last_build_timing(lb_gpu_ivfbq *p, float *ms) { return ivf_last_build_timing(p, ms); }

// ---- what the IVF handles share (lb_ivf_host.h) -------------------------------------------------------------------------
int lb_gpu_ivfbq_add(lb_gpu_ivfbq *p, int64_t n, const float *vectors, const int64_t *ids) { return add_impl(p, n, vectors, ids, false); }
int lb_gpu_ivfbq_add_device(lb_gpu_ivfbq *p, int64_t n, const float *d_vectors, const int64_t *d_ids) { return add_impl(p, n, d_vectors, d_ids, true); }
int lb_gpu_ivfbq_get_centroids(lb_gpu_ivfbq *p, float *out) { return ivf_get_centroids(p, out); }
int lb_gpu_ivfbq_list_sizes(lb_gpu_ivfbq *p, int64_t *sizes) { return ivf_list_sizes(p, sizes); }
int lb_gpu_ivfbq_assignments(lb_gpu_ivfbq *p, int64_t row0, int64_t n, int32_t *lists) { return ivf_assignments(p, row0, n, lists); }
int lb_gpu_ivfbq_search_device_ctx(lb_gpu_ivfbq *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels,
                                   void *stream, const lb_cancel *ctx)
{
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, ivfbq_search_dev);
}
int lb_gpu_ivfbq_search_ctx(lb_gpu_ivfbq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                            const lb_cancel *ctx)
{
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, ivfbq_search_dev);
}
int lb_gpu_ivfbq_search(lb_gpu_ivfbq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels)
{
    return lb_gpu_ivfbq_search_ctx(p, nq, queries, k, nprobe, dist, labels, nullptr);
}
int lb_gpu_ivfbq_last_search_stats(lb_gpu_ivfbq *p, int64_t out[4]) { return ivf_last_search_stats(p, out); }
int lb_gpu_ivfbq_set_profiling(lb_gpu_ivfbq *p, int enable) { return ivf_set_profiling(p, enable); }
int lb_gpu_ivfbq_last_timing(lb_gpu_ivfbq *p, float ms[5]) { return ivf_last_timing(p, ms); }

} // extern "C"
