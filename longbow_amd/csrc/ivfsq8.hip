// ivfsq8.hip -- host side of the lb_gpu_ivfsq8_* entry points of include/longbow_gpu.h: the IVF-SQ8 index, the coarse partition of
// the IVF-Flat handle (ivf.hip) over the codes of the SQ8 handle (sq8.hip).  The new kernels are in kernels_ivfsq8.hip; the coarse
// quantiser is an inner exact f32 index over the centroids, the lists are kernels_ivf.hip's, the codec and the norms
// kernels_sq8.hip's.  The codes stay in insertion order, so under a row filter the visible lists hold rows, as on IVF-Flat.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_ivf_host.h"
#include "lb_ivfsq8.h"

using namespace lb;

struct lb_gpu_ivfsq8 : IvfHandle { // the partition (L2), and under a row filter the visible lists of rows (lb_ivf_host.h)
    int order = 0, stride = 0;
    DevBuf<uint8_t> d_codes;        // [capacity][stride], insertion order, pad bytes zero
    std::vector<float> h_min, h_max; // [dims], fixed at creation
    DevBuf<float> d_par;            // [3][dims]: min, max, scale
    float timing[5] = {0, 0, 0, 0, 0}; // of the last profiled search (under err_mu): probes, plan, the queries' codes, scan, select; ms summed over its batches
    const float *dmin() const { return d_par.get(); }
    const float *dmax() const { return d_par.get() + dims; }
    const float *dscale() const { return d_par.get() + 2 * (size_t)dims; }
};

namespace {

void ivfsq8_grow(lb_gpu_ivfsq8 *p, int64_t need, bool want_ids) { ivf_grow(p, need, want_ids, {{&p->d_codes, (size_t)p->stride, false}}); }

// The handle's share of the add (lb_ivf_host.h: ivf_add).  The vectors are staged piece_rows(dims) rows at a time (64 Mi floats:
// 256 MB of host vectors, 12 bytes of labels and distances a row of a piece) and are not kept: a piece's codes are stored, and
// nothing is derived from the new lists.
int add_impl(lb_gpu_ivfsq8 *p, int64_t n, const float *vectors, const int64_t *ids, bool on_device)
{
    if (!p) return LB_ERR_INVALID_ARG;
    IvfAddSource src{vectors, on_device, p->device, p->dims};
    return ivf_add(
        p, n, vectors, ids, on_device, piece_rows(p->dims), [&](int64_t total, bool want_ids) { ivfsq8_grow(p, total, want_ids); }, src,
        [&](const float *d_rows, int64_t r0, int64_t cnt, int64_t, hipStream_t s) {
            launch_sq8_encode(d_rows, cnt, p->dims, p->dmin(), p->dmax(), p->dscale(), p->d_codes.get() + (size_t)(p->n + r0) * p->stride, s);
        },
        ivf_no_relist);
}

// The handle's call of the search loop (lb_ivf_host.h): exact integer k-NN.  Its middle steps are the queries' codes and their
// norms, a timing slot of their own, and the scan of the probed lists' rows; the selection is the one over integer keys.  The
// lists hold rows and the scan gathers by row, so the visible lists and a call's go through the loop as the IVF-Flat handle's do.
int ivfsq8_search_dev(lb_gpu_ivfsq8 *p, const IvfCall &c)
{
    uint8_t *d_qc = nullptr;
    int32_t *d_qn = nullptr;
    hipStream_t s = c.s;
    return ivf_search(
        p, c, IvfSearchForm{p->timing, 5, kQueryBatch, launch_ivfsq8_select},
        [&](Carve &cv, IvfBatch &, int64_t nb) {
            d_qc = cv.take<uint8_t>((size_t)nb * p->stride);
            d_qn = cv.take<int32_t>((size_t)nb * 4);
        },
        [&](const IvfBatch &b, const IvfWalk &w, auto &&poll, auto &&next) {
            if (!next()) return false; // (the plan's slot ends here)
            launch_sq8_encode(b.Q, b.nq, p->dims, p->dmin(), p->dmax(), p->dscale(), d_qc, s);
            if (!poll()) return false;
            launch_sq8_norms(d_qc, b.nq, p->stride, d_qn, s);
            if (!next()) return false;
            launch_ivfsq8_scan(IvfSq8Scan{b, p->d_codes.get(), p->n, p->stride, d_qc, d_qn}, w.maxlen, s);
            return true;
        });
}


} // namespace

extern "C" {

lb_gpu_ivfsq8 *lb_gpu_ivfsq8_new(int device, int dims, const float *min, const float *max, int order, int nlist, const float *centroids,
                                 int *out_status)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    if (dims <= 0 || !min || !max || order < 0 || order > 1 || nlist <= 0 || !centroids) { st(LB_ERR_INVALID_ARG); return nullptr; }
    // SQ8Config.Validate (scalar_quantization.go:44-49): NaN bounds pass, as on lb_gpu_sq8_set_bounds
    for (int i = 0; i < dims; i++)
        if (min[i] >= max[i]) { st(LB_ERR_INVALID_ARG); return nullptr; }
    if (dims > LB_MAX_DIM || nlist > IVF_MAX_NLIST) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    return ivf_open<lb_gpu_ivfsq8>(device, dims, 0 /* L2 */, order, nlist, centroids, out_status, [&](lb_gpu_ivfsq8 *p) {
        p->order = order;
        p->stride = sq8_stride(dims);
        p->h_min.assign(min, min + dims);
        p->h_max.assign(max, max + dims);
        // NewSQ8Encoder's scale (scalar_quantization.go:75-79), in f32 on the host so that no device division enters
        std::vector<float> par((size_t)3 * dims);
        for (int i = 0; i < dims; i++) {
            const volatile float range = max[i] - min[i];
            par[i] = min[i];
            par[(size_t)dims + i] = max[i];
            par[(size_t)2 * dims + i] = 255.0f / range;
        }
        p->d_par.alloc((size_t)3 * dims);
        LB_HIP(hipMemcpy(p->d_par.get(), par.data(), par.size() * 4, hipMemcpyHostToDevice));
    });
}

void lb_gpu_ivfsq8_free(lb_gpu_ivfsq8 *p) { handle_free(p); }
const char *lb_gpu_ivfsq8_last_error(const lb_gpu_ivfsq8 *p) { return handle_last_error(p); }
int lb_gpu_ivfsq8_dims(const lb_gpu_ivfsq8 *p) { return p ? p->dims : 0; }
int lb_gpu_ivfsq8_order(const lb_gpu_ivfsq8 *p) { return p ? p->order : 0; }
int lb_gpu_ivfsq8_nlist(const lb_gpu_ivfsq8 *p) { return p ? p->part.nlist : 0; }
int64_t lb_gpu_ivfsq8_ntotal(const lb_gpu_ivfsq8 *p) { return handle_ntotal(p); }

int64_t lb_gpu_ivfsq8_hbm_bytes(const lb_gpu_ivfsq8 *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_ivfsq8 *>(p)->mu);
    return (int64_t)(p->d_codes.count() + p->d_par.count() * 4) + p->visible_bytes() + p->part.hbm_bytes();
}

int lb_gpu_ivfsq8_get_bounds(lb_gpu_ivfsq8 *p, float *min, float *max)
{
    if (!p || !min || !max) return LB_ERR_INVALID_ARG;
    std::copy(p->h_min.begin(), p->h_min.end(), min); // (fixed at creation)
    std::copy(p->h_max.begin(), p->h_max.end(), max);
    return LB_OK;
}

int lb_gpu_ivfsq8_reserve(lb_gpu_ivfsq8 *p, int64_t n_total)
{
    return handle_reserve(p, n_total, [](lb_gpu_ivfsq8 *h, int64_t need) { ivfsq8_grow(h, need, h->part.has_ids); });
}

int lb_gpu_ivfsq8_get_codes(lb_gpu_ivfsq8 *p, int64_t row0, int64_t n, uint8_t *codes)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    Lease tmp;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        const uint8_t *src = p->d_codes.get() + (size_t)row0 * p->stride;
        if (p->stride != p->dims) { // strip the pad bytes
            tmp.reset(p->device, (size_t)n * p->dims);
            launch_sq8_restride(src, p->stride, tmp.as<uint8_t>(), p->dims, p->dims, n, p->stream);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(p->stream));
            src = tmp.as<uint8_t>();
        }
        LB_HIP(hipMemcpy(codes, src, (size_t)n * p->dims, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- the row filter (lb_handle.h, lb_ivf_host.h) ------------------------------------------------------------------------
int64_t lb_gpu_ivfsq8_nvisible(const lb_gpu_ivfsq8 *p) { return filter_nvisible(p); }
int lb_gpu_ivfsq8_set_filter(lb_gpu_ivfsq8 *p, const uint8_t *mask, int64_t n) { return ivf_set_filter(p, mask, n); }
int lb_gpu_ivfsq8_filter_int64(lb_gpu_ivfsq8 *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                               int64_t validity_offset, int combine)
{
    return ivf_filter_column<int64_t>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivfsq8_filter_float32(lb_gpu_ivfsq8 *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                                 int64_t validity_offset, int combine)
{
    return ivf_filter_column<float>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivfsq8_last_build_timing(lb_gpu_ivfsq8 *p, float *ms) { return ivf_last_build_timing(p, ms); }

// ---- removal and compaction (lb_ivf_host.h, lb_remove.h) ----------------------------------------------------------------
int lb_gpu_ivfsq8_remove(lb_gpu_ivfsq8 *p, int64_t n, const int64_t *labels, int64_t *n_removed) { return ivf_remove(p, n, labels, n_removed); }
int lb_gpu_ivfsq8_remove_device(lb_gpu_ivfsq8 *p, int64_t n, const int64_t *d_labels, int64_t *n_removed)
{
    return ivf_remove_device(p, n, d_labels, n_removed);
}
int lb_gpu_ivfsq8_remove_rows(lb_gpu_ivfsq8 *p, int64_t n, const int64_t *rows, int64_t *n_removed) { return ivf_remove_rows(p, n, rows, n_removed); }
int64_t lb_gpu_ivfsq8_nlive(const lb_gpu_ivfsq8 *p) { return ivf_nlive(p); }
int64_t lb_gpu_ivfsq8_ndeleted(const lb_gpu_ivfsq8 *p) { return ivf_ndeleted(p); }
// (the codes are the rows that move, `stride` bytes each with their zero pad bytes; the scan reads them in insertion order, so
// nothing else is derived from them)
int lb_gpu_ivfsq8_compact(lb_gpu_ivfsq8 *p, int64_t *old_rows, int64_t cap)
{
    if (!p) return LB_ERR_INVALID_ARG;
    return ivf_compact(p, [p] { return static_cast<void *>(p->d_codes.get()); }, (size_t)p->stride, old_rows, cap, ivf_no_relist);
}

// ---- what the IVF handles share (lb_ivf_host.h) -------------------------------------------------------------------------
int lb_gpu_ivfsq8_add(lb_gpu_ivfsq8 *p, int64_t n, const float *vectors, const int64_t *ids) { return add_impl(p, n, vectors, ids, false); }
int lb_gpu_ivfsq8_add_device(lb_gpu_ivfsq8 *p, int64_t n, const float *d_vectors, const int64_t *d_ids) { return add_impl(p, n, d_vectors, d_ids, true); }
int lb_gpu_ivfsq8_get_centroids(lb_gpu_ivfsq8 *p, float *out) { return ivf_get_centroids(p, out); }
int lb_gpu_ivfsq8_list_sizes(lb_gpu_ivfsq8 *p, int64_t *sizes) { return ivf_list_sizes(p, sizes); }
int lb_gpu_ivfsq8_assignments(lb_gpu_ivfsq8 *p, int64_t row0, int64_t n, int32_t *lists) { return ivf_assignments(p, row0, n, lists); }
int lb_gpu_ivfsq8_search_device_ctx(lb_gpu_ivfsq8 *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels,
                                    void *stream, const lb_cancel *ctx)
{
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, ivfsq8_search_dev);
}
int lb_gpu_ivfsq8_search_ctx(lb_gpu_ivfsq8 *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                             const lb_cancel *ctx)
{
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, ivfsq8_search_dev);
}
int lb_gpu_ivfsq8_search(lb_gpu_ivfsq8 *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels)
{
    return lb_gpu_ivfsq8_search_ctx(p, nq, queries, k, nprobe, dist, labels, nullptr);
}
// the same searches under a row bitmap given with the call (a NULL bitmap: the plain search)
int lb_gpu_ivfsq8_search_bitmap_device_ctx(lb_gpu_ivfsq8 *p, int64_t nq, const float *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                           int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, ivfsq8_search_dev,
                                 CallBitmap{d_bitmap, nbits, stride_bytes, true});
}
int lb_gpu_ivfsq8_search_bitmap_ctx(lb_gpu_ivfsq8 *p, int64_t nq, const float *queries, int k, int nprobe, const uint8_t *bitmap, int64_t nbits,
                                    int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, ivfsq8_search_dev, CallBitmap{bitmap, nbits, stride_bytes, false});
}
int lb_gpu_ivfsq8_last_search_stats(lb_gpu_ivfsq8 *p, int64_t out[4]) { return ivf_last_search_stats(p, out); }
int lb_gpu_ivfsq8_set_profiling(lb_gpu_ivfsq8 *p, int enable) { return ivf_set_profiling(p, enable); }
int lb_gpu_ivfsq8_last_timing(lb_gpu_ivfsq8 *p, float ms[5]) { return ivf_last_timing(p, ms); }

} // extern "C"
