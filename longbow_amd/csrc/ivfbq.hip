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
    DevBuf<uint8_t> d_codes;        // [capacity][W] u64 words, insertion order: what get_codes returns
    // the list-major codes are built for all rows by every add, with the lists, into the pair that is not in use
    DevBuf<uint8_t> d_lcodes[2];    // [capacity][W] u64 words: lcodes[pos] = codes[list[pos]]
    float timing[5] = {0, 0, 0, 0, 0}; // of the last profiled search (under err_mu): probes, plan, the queries' codes, scan, select; ms summed over its batches
    size_t row_bytes(int64_t rows = 1) const { return (size_t)rows * (size_t)W * 8; }
};

namespace {

void ivfbq_grow(lb_gpu_ivfbq *p, int64_t need, bool want_ids)
{
    ivf_grow(p, need, want_ids, {{&p->d_codes, p->row_bytes(), false}, {p->d_lcodes, p->row_bytes(), true}});
}

// The handle's share of the add (lb_ivf_host.h: ivf_add).  The vectors are staged piece_rows(dims) rows at a time (64 Mi floats:
// 256 MB of host vectors, 12 bytes of labels and distances a row of a piece) and are not kept: a piece's codes are stored, and
// from the new lists the codes in list order are derived, into the pair not in use.
int add_impl(lb_gpu_ivfbq *p, int64_t n, const float *vectors, const int64_t *ids, bool on_device)
{
    if (!p) return LB_ERR_INVALID_ARG;
    IvfAddSource src{vectors, on_device, p->device, p->dims};
    return ivf_add(
        p, n, vectors, ids, on_device, piece_rows(p->dims), [&](int64_t total, bool want_ids) { ivfbq_grow(p, total, want_ids); }, src,
        [&](const float *d_rows, int64_t r0, int64_t cnt, int64_t, hipStream_t s) {
            launch_bq_encode(d_rows, cnt, p->dims, reinterpret_cast<uint64_t *>(p->d_codes.get() + p->row_bytes(p->n + r0)), s);
        },
        [&](int nxt, int64_t total, hipStream_t s) {
            launch_ivfpq_permute(p->d_codes.get(), p->part.d_list[nxt].get(), total, (int)p->row_bytes(), p->d_lcodes[nxt].get(), s);
        });
}

// The handle's call of the search loop (lb_ivf_host.h): exact Hamming k-NN.  Its middle steps are the queries' codes, a timing
// slot of their own, and the scan of the list-major codes, in its `_visible` form where the batch walks other lists than those of
// all rows (w.subset: positions bounded by w.entries); the selection is the one over integer keys.
int ivfbq_search_dev(lb_gpu_ivfbq *p, const IvfCall &c)
{
    const IvfPartition &P = p->part;
    const uint64_t *lcodes = reinterpret_cast<const uint64_t *>(p->d_lcodes[P.cur].get());
    const uint32_t *rows = P.d_list[P.cur].get();
    uint64_t *d_qc = nullptr;
    hipStream_t s = c.s;
    return ivf_search(
        p, c, IvfSearchForm{p->timing, 5, kQueryBatch, launch_ivfsq8_select},
        [&](Carve &cv, IvfBatch &, int64_t nb) { d_qc = cv.take<uint64_t>(p->row_bytes(nb)); },
        [&](const IvfBatch &b, const IvfWalk &w, auto &&, auto &&next) {
            if (!next()) return false; // (the plan's slot ends here)
            launch_bq_encode(b.Q, b.nq, p->dims, d_qc, s);
            if (!next()) return false;
            const IvfBqScan scan{b, lcodes, rows, p->n, p->W, d_qc, w.subset ? w.entries : 0};
            if (w.subset) launch_ivfbq_scan_visible(scan, w.maxlen, s);
            else launch_ivfbq_scan(scan, w.maxlen, s);
            return true;
        });
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
    return (int64_t)(p->d_codes.count() + p->d_lcodes[0].count() + p->d_lcodes[1].count()) + p->visible_bytes() + p->part.hbm_bytes();
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
        LB_HIP(hipMemcpy(codes, p->d_codes.get() + p->row_bytes(row0), p->row_bytes(n), hipMemcpyDeviceToHost));
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
