// ivf.hip -- host side of the lb_gpu_ivf_* entry points of include/longbow_gpu.h: the IVF-Flat index the reference names as
// a plug-point (internal/store/pluggable_index.go:18-25,100-104; its adapter, pluggable_index_adapters.go:116-223, is a stub).
// The kernels are in kernels_ivf.hip, those of a row bitmap given with a search call in kernels_ivf_call.hip, the list scan over float16 rows in kernels_ivf_f16.hip, the one over int8 rows in
// kernels_ivf_i8.hip; the coarse quantiser is an inner exact f32 index over the centroids, whatever the rows' element type.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_ivf_f16.h"
#include "lb_ivf_host.h"
#include "lb_ivf_i8.h"

using namespace lb;

enum { DT_F32 = 0, DT_F16 = 1, DT_I8 = 2 }; // simd.DataType, what lb_gpu_ivf_dtype returns

struct lb_gpu_ivf : IvfHandle { // the partition, and under a row filter the visible lists of rows (lb_ivf_host.h)
    int metric = 0, order = 0;
    int dtype = DT_F32;             // the rows' element type, fixed at creation (lb_gpu_ivf_new, _new_f16, _new_i8)
    DevBuf<uint8_t> d_rows;         // [capacity][dims] of that type (float16: IEEE binary16), insertion order; no wider copy is held
    size_t row_bytes() const { return (size_t)dims * (dtype == DT_I8 ? 1 : dtype == DT_F16 ? 2 : 4); }
    template <class E> const E *rows() const { return reinterpret_cast<const E *>(d_rows.get()); }
    float timing[4] = {0, 0, 0, 0};  // of the last profiled search (under err_mu): probes, plan, scan, select; ms summed over its batches
};

namespace {

// rows of an add to a float16 or int8 handle that are widened to f32 and assigned at a time: an add never needs an f32 copy of itself
constexpr int64_t IVF_WIDEN_ASSIGN_ROWS = 65536;

void ivf_flat_grow(lb_gpu_ivf *p, int64_t need, bool want_ids) { ivf_grow(p, need, want_ids, {{&p->d_rows, p->row_bytes(), false}}); }

// the error a handle reports to an entry point of another element type, as the flat index does (index.hip)
int wrong_dtype(lb_gpu_ivf *p)
{
    p->set_error("%s", p->dtype == DT_I8    ? "this index holds int8 rows: use the _i8 entry point"
                       : p->dtype == DT_F16 ? "this index holds float16 rows: use the _f16 entry point"
                                            : "this index holds float32 rows: use the float32 entry point");
    return LB_ERR_INVALID_ARG;
}
// dtype: the element type of the rows an add entry point takes
int dtype_mismatch(lb_gpu_ivf *p, int dtype) { return p->dtype == dtype ? (int)LB_OK : wrong_dtype(p); }
// i8: the element type of the queries a search entry point takes.  An int8 handle takes int8 queries and nothing else; the
// other two take f32 queries.
int query_mismatch(lb_gpu_ivf *p, bool i8)
{
    if (!p) return LB_ERR_INVALID_ARG;
    return (p->dtype == DT_I8) == i8 ? (int)LB_OK : wrong_dtype(p);
}

// The handle's share of the add (lb_ivf_host.h: ivf_add).  vectors: n rows of the entry point's element type (DT_F16: uint16_t bit
// patterns), on the host or on the device.  They are stored as they come, all of them ahead of the first piece; a float32 handle
// assigns them in one piece from where they are stored, the others IVF_WIDEN_ASSIGN_ROWS at a time, each piece widened into an
// f32 scratch that the coarse search reads.  Nothing else is stored and nothing is derived from the new lists.
int add_impl(lb_gpu_ivf *p, int64_t n, const void *vectors, const int64_t *ids, bool on_device, int dtype)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (const int st = dtype_mismatch(p, dtype)) return st;
    Lease wide;
    const size_t rb = p->row_bytes();
    return ivf_add(
        p, n, vectors, ids, on_device, dtype == DT_F32 ? n : IVF_WIDEN_ASSIGN_ROWS,
        [&](int64_t total, bool want_ids) { ivf_flat_grow(p, total, want_ids); },
        [&](int64_t r0, int64_t cnt, int64_t piece, hipStream_t s) -> const float * {
            uint8_t *d_new = p->d_rows.get() + (size_t)p->n * rb;
            if (r0 == 0) LB_HIP(hipMemcpyAsync(d_new, vectors, (size_t)n * rb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
            if (dtype == DT_F32) return reinterpret_cast<const float *>(d_new);
            if (r0 == 0) wide.reset(p->device, (size_t)piece * p->dims * 4);
            (dtype == DT_I8 ? launch_widen_i8 : launch_widen_f16)(d_new + (size_t)r0 * rb, wide.as<float>(), cnt * p->dims, s);
            return wide.as<float>();
        },
        ivf_no_store, ivf_no_relist);
}

// The handle's call of the search loop (lb_ivf_host.h): its middle steps are the queries' norms under cosine, inside the plan's
// timing slot, and the scan of the rows.  d_q8: on an int8 handle the call's int8 queries, c.queries being those widened to f32;
// the scan reads the int8 ones, a batch's at the offset of its b.Q in c.queries.
int ivf_search_rows(lb_gpu_ivf *p, const IvfCall &c, const int8_t *d_q8)
{
    float *d_qna = nullptr;
    return ivf_search(
        p, c, IvfSearchForm{p->timing, 4},
        [&](Carve &cv, IvfBatch &b, int64_t nb) {
            b.X = p->dtype == DT_F32 ? p->rows<float>() : nullptr; // (the plan and the selection read no rows)
            b.qna = d_qna = cv.take<float>((size_t)nb * 4);
        },
        [&](const IvfBatch &b, const IvfWalk &w, auto &&poll, auto &&next) {
            if (p->metric == METRIC_COS) {
                if (!poll()) return false;
                launch_query_norms(p->order, b.Q, nullptr, b.nq, p->dims, d_qna, c.s);
            }
            if (!next()) return false;
            if (p->dtype == DT_I8) launch_ivf_scan_i8(p->metric, IvfI8Scan{b, p->rows<int8_t>(), d_q8 + (b.Q - c.queries)}, w.maxlen, c.s);
            else if (p->dtype == DT_F16) launch_ivf_scan_f16(p->metric, p->order, IvfF16Scan{b, p->rows<_Float16>()}, w.maxlen, c.s);
            else launch_ivf_scan(p->metric, p->order, b, w.maxlen, c.s);
            return true;
        });
}

// A float32 or float16 handle's search of f32 queries
int ivf_search_dev(lb_gpu_ivf *p, const IvfCall &c) { return ivf_search_rows(p, c, nullptr); }

// An int8 handle's: the call's int8 queries are widened once into `wide` (the caller's lease, declared outside its guard), which
// is what the coarse index probes with; ctx is polled before that launch as before every other.
int ivf_search_i8_dev(lb_gpu_ivf *p, const IvfCallOf<int8_t> &c, Lease &wide)
{
    wide.reset(p->device, (size_t)c.nq * p->dims * 4);
    if (const int st = ctx_state(c.ctx)) return ctx_fail(p, st);
    launch_widen_i8(c.queries, wide.as<float>(), c.nq * p->dims, c.s);
    return ivf_search_rows(p, IvfCall{c.nq, wide.as<float>(), c.k, c.nprobe, c.dist, c.labels, c.s, c.ctx, c.sc, c.filter}, c.queries);
}

} // namespace

extern "C" {

static lb_gpu_ivf *ivf_new(int device, int dim, int metric, int order, int nlist, const float *centroids, int *out_status, int dtype)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    if (dim <= 0 || metric < 0 || metric > 2 || order < 0 || order > 1 || nlist <= 0 || !centroids) { st(LB_ERR_INVALID_ARG); return nullptr; }
    if (dim > LB_MAX_DIM || nlist > IVF_MAX_NLIST) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    // int8 rows: lb_gpu_index_new_i8's rules, for its reasons (no cosine kernel in the reference; exact dot chains)
    if (dtype == DT_I8 && (metric == LB_METRIC_COSINE || (metric == LB_METRIC_DOT && dim / 4 + dim % 4 > 1024))) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    return ivf_open<lb_gpu_ivf>(device, dim, metric, order, nlist, centroids, out_status, [&](lb_gpu_ivf *p) {
        p->metric = metric;
        p->order = order;
        p->dtype = dtype;
    });
}

lb_gpu_ivf *lb_gpu_ivf_new(int device, int dim, int metric, int order, int nlist, const float *centroids, int *out_status)
{
    return ivf_new(device, dim, metric, order, nlist, centroids, out_status, DT_F32);
}
lb_gpu_ivf *lb_gpu_ivf_new_f16(int device, int dim, int metric, int order, int nlist, const float *centroids, int *out_status)
{
    return ivf_new(device, dim, metric, order, nlist, centroids, out_status, DT_F16);
}
lb_gpu_ivf *lb_gpu_ivf_new_i8(int device, int dim, int metric, int order, int nlist, const float *centroids, int *out_status)
{
    return ivf_new(device, dim, metric, order, nlist, centroids, out_status, DT_I8);
}
int lb_gpu_ivf_dtype(const lb_gpu_ivf *p) { return p ? p->dtype : 0; }

void lb_gpu_ivf_free(lb_gpu_ivf *p) { handle_free(p); }
const char *lb_gpu_ivf_last_error(const lb_gpu_ivf *p) { return handle_last_error(p); }
int lb_gpu_ivf_dim(const lb_gpu_ivf *p) { return p ? p->dims : 0; }
int lb_gpu_ivf_metric(const lb_gpu_ivf *p) { return p ? p->metric : 0; }
int lb_gpu_ivf_order(const lb_gpu_ivf *p) { return p ? p->order : 0; }
int lb_gpu_ivf_nlist(const lb_gpu_ivf *p) { return p ? p->part.nlist : 0; }
int64_t lb_gpu_ivf_ntotal(const lb_gpu_ivf *p) { return handle_ntotal(p); }

int64_t lb_gpu_ivf_hbm_bytes(const lb_gpu_ivf *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_ivf *>(p)->mu);
    return (int64_t)p->d_rows.count() + p->visible_bytes() + p->part.hbm_bytes();
}

int lb_gpu_ivf_reserve(lb_gpu_ivf *p, int64_t n_total)
{
    return handle_reserve(p, n_total, [](lb_gpu_ivf *h, int64_t need) { ivf_flat_grow(h, need, h->part.has_ids); });
}

// ---- the row filter (lb_handle.h) ---------------------------------------------------------------------------------------
int64_t lb_gpu_ivf_nvisible(const lb_gpu_ivf *p) { return filter_nvisible(p); }
int lb_gpu_ivf_set_filter(lb_gpu_ivf *p, const uint8_t *mask, int64_t n) { return ivf_set_filter(p, mask, n); }
int lb_gpu_ivf_filter_int64(lb_gpu_ivf *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                            int64_t validity_offset, int combine)
{
    return ivf_filter_column<int64_t>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivf_filter_float32(lb_gpu_ivf *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                              int64_t validity_offset, int combine)
{
    return ivf_filter_column<float>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivf_last_build_timing(lb_gpu_ivf *p, float *ms) { return ivf_last_build_timing(p, ms); }

// ---- removal and compaction (lb_ivf_host.h, lb_remove.h) ----------------------------------------------------------------
int lb_gpu_ivf_remove(lb_gpu_ivf *p, int64_t n, const int64_t *labels, int64_t *n_removed) { return ivf_remove(p, n, labels, n_removed); }
int lb_gpu_ivf_remove_device(lb_gpu_ivf *p, int64_t n, const int64_t *d_labels, int64_t *n_removed)
{
    return ivf_remove_device(p, n, d_labels, n_removed);
}
int lb_gpu_ivf_remove_rows(lb_gpu_ivf *p, int64_t n, const int64_t *rows, int64_t *n_removed) { return ivf_remove_rows(p, n, rows, n_removed); }
int64_t lb_gpu_ivf_nlive(const lb_gpu_ivf *p) { return ivf_nlive(p); }
int64_t lb_gpu_ivf_ndeleted(const lb_gpu_ivf *p) { return ivf_ndeleted(p); }
// (the rows of the handle's element type move as bytes; the buffer is read under the lock that ivf_compact takes: through the getter)
int lb_gpu_ivf_compact(lb_gpu_ivf *p, int64_t *old_rows, int64_t cap)
{
    if (!p) return LB_ERR_INVALID_ARG;
    return ivf_compact(p, [p] { return static_cast<void *>(p->d_rows.get()); }, p->row_bytes(), old_rows, cap, ivf_no_relist);
}

// ---- what the IVF handles share (lb_ivf_host.h) -------------------------------------------------------------------------
int lb_gpu_ivf_add(lb_gpu_ivf *p, int64_t n, const float *vectors, const int64_t *ids) { return add_impl(p, n, vectors, ids, false, DT_F32); }
int lb_gpu_ivf_add_device(lb_gpu_ivf *p, int64_t n, const float *d_vectors, const int64_t *d_ids) { return add_impl(p, n, d_vectors, d_ids, true, DT_F32); }
int lb_gpu_ivf_add_f16(lb_gpu_ivf *p, int64_t n, const uint16_t *vectors, const int64_t *ids) { return add_impl(p, n, vectors, ids, false, DT_F16); }
int lb_gpu_ivf_add_f16_device(lb_gpu_ivf *p, int64_t n, const uint16_t *d_vectors, const int64_t *d_ids)
{
    return add_impl(p, n, d_vectors, d_ids, true, DT_F16);
}
int lb_gpu_ivf_add_i8(lb_gpu_ivf *p, int64_t n, const int8_t *vectors, const int64_t *ids) { return add_impl(p, n, vectors, ids, false, DT_I8); }
int lb_gpu_ivf_add_i8_device(lb_gpu_ivf *p, int64_t n, const int8_t *d_vectors, const int64_t *d_ids)
{
    return add_impl(p, n, d_vectors, d_ids, true, DT_I8);
}
int lb_gpu_ivf_get_centroids(lb_gpu_ivf *p, float *out) { return ivf_get_centroids(p, out); }
int lb_gpu_ivf_list_sizes(lb_gpu_ivf *p, int64_t *sizes) { return ivf_list_sizes(p, sizes); }
int lb_gpu_ivf_assignments(lb_gpu_ivf *p, int64_t row0, int64_t n, int32_t *lists) { return ivf_assignments(p, row0, n, lists); }
// the searches, plain and under a row bitmap given with the call: one pair of bodies, a plain search being the one without a bitmap
static int search_device(lb_gpu_ivf *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels, void *stream,
                         const lb_cancel *ctx, const CallBitmap &b)
{
    if (const int st = query_mismatch(p, false)) return st;
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, ivf_search_dev, b);
}
static int search_host(lb_gpu_ivf *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels, const lb_cancel *ctx,
                       const CallBitmap &b)
{
    if (const int st = query_mismatch(p, false)) return st;
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, ivf_search_dev, b);
}
// the int8 handle's: int8 queries, widened once for the coarse index
static int search_i8_device(lb_gpu_ivf *p, int64_t nq, const int8_t *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels, void *stream,
                            const lb_cancel *ctx, const CallBitmap &b)
{
    if (const int st = query_mismatch(p, true)) return st;
    Lease wide;
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx,
                                 [&](lb_gpu_ivf *h, const IvfCallOf<int8_t> &c) { return ivf_search_i8_dev(h, c, wide); }, b);
}
static int search_i8_host(lb_gpu_ivf *p, int64_t nq, const int8_t *queries, int k, int nprobe, float *dist, int64_t *labels, const lb_cancel *ctx,
                          const CallBitmap &b)
{
    if (const int st = query_mismatch(p, true)) return st;
    Lease wide;
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx,
                          [&](lb_gpu_ivf *h, const IvfCallOf<int8_t> &c) { return ivf_search_i8_dev(h, c, wide); }, b);
}
int lb_gpu_ivf_search_device_ctx(lb_gpu_ivf *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels,
                                 void *stream, const lb_cancel *ctx)
{
    return search_device(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, CallBitmap{});
}
int lb_gpu_ivf_search_ctx(lb_gpu_ivf *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return search_host(p, nq, queries, k, nprobe, dist, labels, ctx, CallBitmap{});
}
int lb_gpu_ivf_search(lb_gpu_ivf *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels)
{
    return lb_gpu_ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, nullptr);
}
int lb_gpu_ivf_search_i8_device_ctx(lb_gpu_ivf *p, int64_t nq, const int8_t *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels,
                                    void *stream, const lb_cancel *ctx)
{
    return search_i8_device(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, CallBitmap{});
}
int lb_gpu_ivf_search_i8_ctx(lb_gpu_ivf *p, int64_t nq, const int8_t *queries, int k, int nprobe, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return search_i8_host(p, nq, queries, k, nprobe, dist, labels, ctx, CallBitmap{});
}
int lb_gpu_ivf_search_i8(lb_gpu_ivf *p, int64_t nq, const int8_t *queries, int k, int nprobe, float *dist, int64_t *labels)
{
    return lb_gpu_ivf_search_i8_ctx(p, nq, queries, k, nprobe, dist, labels, nullptr);
}
int lb_gpu_ivf_search_bitmap_device_ctx(lb_gpu_ivf *p, int64_t nq, const float *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                        int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return search_device(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, CallBitmap{d_bitmap, nbits, stride_bytes, true});
}
int lb_gpu_ivf_search_bitmap_ctx(lb_gpu_ivf *p, int64_t nq, const float *queries, int k, int nprobe, const uint8_t *bitmap, int64_t nbits,
                                 int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return search_host(p, nq, queries, k, nprobe, dist, labels, ctx, CallBitmap{bitmap, nbits, stride_bytes, false});
}
int lb_gpu_ivf_search_i8_bitmap_device_ctx(lb_gpu_ivf *p, int64_t nq, const int8_t *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                           int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream,
                                           const lb_cancel *ctx)
{
    return search_i8_device(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, CallBitmap{d_bitmap, nbits, stride_bytes, true});
}
int lb_gpu_ivf_search_i8_bitmap_ctx(lb_gpu_ivf *p, int64_t nq, const int8_t *queries, int k, int nprobe, const uint8_t *bitmap, int64_t nbits,
                                    int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return search_i8_host(p, nq, queries, k, nprobe, dist, labels, ctx, CallBitmap{bitmap, nbits, stride_bytes, false});
}
int lb_gpu_ivf_last_search_stats(lb_gpu_ivf *p, int64_t out[4]) { return ivf_last_search_stats(p, out); }
int lb_gpu_ivf_set_profiling(lb_gpu_ivf *p, int enable) { return ivf_set_profiling(p, enable); }
int lb_gpu_ivf_last_timing(lb_gpu_ivf *p, float ms[4]) { return ivf_last_timing(p, ms); }

} // extern "C"
