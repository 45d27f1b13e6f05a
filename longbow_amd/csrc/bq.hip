// bq.hip -- host side of the lb_gpu_bq_* entry points of include/longbow_gpu.h: store.BQEncoder
// (internal/store/binary_quantization.go) and the exact Hamming k-NN over its codes.  The kernels are in kernels_bq.hip.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_handle.h"

using namespace lb;

struct lb_gpu_bq : FilteredHandle { // searches and reads share mu; adds, reserve and the filter calls take it alone
    int W = 0;
    DevBuf<uint64_t> d_codes;
};

namespace {

constexpr int64_t kQueryBatch = 1024; // queries per pass of the selection: bounds its scratch (33 MB of histograms at W = 128)

void bq_grow(lb_gpu_bq *p, int64_t need)
{
    if (need <= p->capacity) return;
    const int64_t cap = grow_capacity(p->capacity, need, (size_t)p->W * 8);
    DevBuf<uint64_t> nc;
    nc.alloc((size_t)cap * p->W);
    if (p->n > 0) LB_HIP(hipMemcpy(nc.get(), p->d_codes.get(), (size_t)p->n * p->W * 8, hipMemcpyDeviceToDevice));
    p->filter.grow(p->n, cap);
    p->d_codes = std::move(nc);
    p->capacity = cap;
}

// Exact k-NN of nq device-resident query codes over the visible rows; the caller holds the reader lock, has made the device
// current and has checked the arguments.  ctx is polled before every launch.  The scratch is leased into the caller's `sc`, declared outside the
// caller's guard as lb_handle.h asks of every pooled buffer.
int bq_search_codes_dev(lb_gpu_bq *p, int64_t nq, const uint64_t *d_Q, int k, float *d_dist, int64_t *d_labels, hipStream_t s,
                        const lb_cancel *ctx, Lease &sc)
{
    BqSearch a{};
    const RowView v = p->filter.view(p->n);
    a.codes = p->d_codes.get();
    a.n = v.n;
    a.rowmap = v.rowmap;
    a.W = p->W;
    a.k = k;
    countsel_plan(a.n, BQ_MAX_BLOCKS, &a.nblk, &a.tpb);
    const size_t nbins = (size_t)64 * p->W + 1;
    const int64_t nb = std::min(nq, kQueryBatch);
    auto layout = [&](Carve c) {
        a.hist = c.take<uint32_t>((size_t)nb * nbins * 4);
        a.thr = c.take<uint32_t>((size_t)nb * 8);
        a.cnt = c.take<uint32_t>((size_t)nb * std::max(a.nblk, 1) * 8);
        a.tot = c.take<uint32_t>((size_t)nb * 4);
        a.keys = c.take<uint64_t>((size_t)nb * k * 8);
        return c.off;
    };
    lease_layout(sc, p->device, layout);
    int cancelled = 0;
    auto go = [&]() { // false: the context fired, nothing more is enqueued
        cancelled = ctx_state(ctx);
        return cancelled == 0;
    };
    for (int64_t q0 = 0; q0 < nq && !cancelled; q0 += nb) {
        a.Q = d_Q + (size_t)q0 * p->W;
        a.nq = (int)std::min(nb, nq - q0);
        if (a.n > 0) {
            if (!go()) break;
            LB_HIP(hipMemsetAsync(a.hist, 0, (size_t)a.nq * nbins * 4, s));
            launch_bq_hist(a, s);
            if (!go()) break;
            launch_bq_thresh(a, s);
            if (!go()) break;
            launch_bq_count(a, s);
            if (!go()) break;
            launch_countsel_scan(a, s);
            if (!go()) break;
            launch_bq_emit(a, s);
        }
        if (!go()) break;
        launch_countsel_finish(a, d_dist + (size_t)q0 * k, d_labels + (size_t)q0 * k, s, v.rowmap);
    }
    LB_LAUNCH_CHECK();
    LB_HIP(hipStreamSynchronize(s));
    return cancelled ? ctx_fail(p, cancelled) : LB_OK;
}

// host queries (f32 rows, or codes when `coded`) -> search -> results back
int host_search(lb_gpu_bq *p, int64_t nq, const void *queries, bool coded, int k, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    const int rc = knn_args(p, nq, queries, k, dist, labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    return host_knn(
        p, nq, (size_t)p->W * 8, k, dist, labels,
        [&](Lease &dq, Lease &dv, hipStream_t s) {
            if (coded) {
                LB_HIP(hipMemcpyAsync(dq.p, queries, (size_t)nq * p->W * 8, hipMemcpyHostToDevice, s));
                return;
            }
            dv.reset(p->device, (size_t)nq * p->dims * 4);
            LB_HIP(hipMemcpyAsync(dv.p, queries, (size_t)nq * p->dims * 4, hipMemcpyHostToDevice, s));
            launch_bq_encode(dv.as<float>(), nq, p->dims, dq.as<uint64_t>(), s);
        },
        [&](Lease &dq, float *d_dist, int64_t *d_labels, hipStream_t s, Lease &sc) {
            return bq_search_codes_dev(p, nq, dq.as<uint64_t>(), k, d_dist, d_labels, s, ctx, sc);
        });
}

int add_codes_impl(lb_gpu_bq *p, int64_t n, const uint64_t *codes, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_fit(p, p->n, n)) return st;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        bq_grow(p, p->n + n);
        LB_HIP(hipMemcpy(p->d_codes.get() + (size_t)p->n * p->W, codes, (size_t)n * p->W * 8,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        p->filter.on_append(p->n, p->n + n, p->stream);
        p->n += n;
        return LB_OK;
    });
}

} // namespace

extern "C" {

lb_gpu_bq *lb_gpu_bq_new(int device, int dims, int *out_status)
{
    return handle_new<lb_gpu_bq>(device, dims, out_status, [](lb_gpu_bq *p) { p->W = (p->dims + 63) / 64; });
}

void lb_gpu_bq_free(lb_gpu_bq *p) { handle_free(p); }
const char *lb_gpu_bq_last_error(const lb_gpu_bq *p) { return handle_last_error(p); }
int lb_gpu_bq_dims(const lb_gpu_bq *p) { return p ? p->dims : 0; }
int lb_gpu_bq_words(const lb_gpu_bq *p) { return p ? p->W : 0; }
int64_t lb_gpu_bq_ntotal(const lb_gpu_bq *p) { return handle_ntotal(p); }
int lb_gpu_bq_reserve(lb_gpu_bq *p, int64_t n_total) { return handle_reserve(p, n_total, bq_grow); }

// ---- the row filter (lb_handle.h) ---------------------------------------------------------------------------------------
int64_t lb_gpu_bq_nvisible(const lb_gpu_bq *p) { return filter_nvisible(p); }
int lb_gpu_bq_set_filter(lb_gpu_bq *p, const uint8_t *mask, int64_t n) { return filter_set(p, mask, n); }
int lb_gpu_bq_filter_int64(lb_gpu_bq *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                           int64_t validity_offset, int combine)
{
    return filter_column<int64_t>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_bq_filter_float32(lb_gpu_bq *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                             int64_t validity_offset, int combine)
{
    return filter_column<float>(p, column, n, value, op, validity, validity_offset, combine);
}

int lb_gpu_bq_add_codes(lb_gpu_bq *p, int64_t n, const uint64_t *codes) { return add_codes_impl(p, n, codes, false); }
int lb_gpu_bq_add_codes_device(lb_gpu_bq *p, int64_t n, const uint64_t *d_codes) { return add_codes_impl(p, n, d_codes, true); }

int lb_gpu_bq_get_codes(lb_gpu_bq *p, int64_t row0, int64_t n, uint64_t *codes)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        LB_HIP(hipMemcpy(codes, p->d_codes.get() + (size_t)row0 * p->W, (size_t)n * p->W * 8, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- Encode / Decode -----------------------------------------------------------------------------------------------
// (takes no lock: it reads nothing of the handle that changes after lb_gpu_bq_new)
int lb_gpu_bq_encode_device(lb_gpu_bq *p, int64_t n, const float *d_vectors, uint64_t *d_codes, void *stream)
{
    if (!p || n < 0 || (n > 0 && (!d_vectors || !d_codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        launch_bq_encode(d_vectors, n, p->dims, d_codes, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

int lb_gpu_bq_encode(lb_gpu_bq *p, int64_t n, const float *vectors, uint64_t *codes)
{
    if (!p || n < 0 || (n > 0 && (!vectors || !codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    return host_codec(p, n, vectors, (size_t)p->dims * 4, codes, (size_t)p->W * 8, [&](void *dv, void *dc, int64_t cnt) {
        return lb_gpu_bq_encode_device(p, cnt, static_cast<float *>(dv), static_cast<uint64_t *>(dc), nullptr);
    });
}

int lb_gpu_bq_add_vectors_device(lb_gpu_bq *p, int64_t n, const float *d_vectors)
{
    if (!p || n < 0 || (n > 0 && !d_vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_fit(p, p->n, n)) return st;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        bq_grow(p, p->n + n);
        launch_bq_encode(d_vectors, n, p->dims, p->d_codes.get() + (size_t)p->n * p->W, p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(p->stream));
        p->filter.on_append(p->n, p->n + n, p->stream);
        p->n += n;
        return LB_OK;
    });
}

int lb_gpu_bq_add_vectors(lb_gpu_bq *p, int64_t n, const float *vectors)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_fit(p, p->n, n)) return st;
    Lease dv;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        bq_grow(p, p->n + n);
        const int64_t piece = std::min(n, piece_rows(p->dims));
        dv.reset(p->device, (size_t)piece * p->dims * 4);
        for (int64_t r0 = 0; r0 < n; r0 += piece) { // the rows become visible (p->n) only once all are encoded
            const int64_t cnt = std::min(piece, n - r0);
            LB_HIP(hipMemcpy(dv.p, vectors + (size_t)r0 * p->dims, (size_t)cnt * p->dims * 4, hipMemcpyHostToDevice));
            launch_bq_encode(dv.as<float>(), cnt, p->dims, p->d_codes.get() + (size_t)(p->n + r0) * p->W, p->stream);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(p->stream));
        }
        p->filter.on_append(p->n, p->n + n, p->stream);
        p->n += n;
        return LB_OK;
    });
}

int lb_gpu_bq_decode(lb_gpu_bq *p, int64_t n, const uint64_t *codes, float *vectors)
{
    if (!p || n < 0 || (n > 0 && (!vectors || !codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    return host_codec(p, n, codes, (size_t)p->W * 8, vectors, (size_t)p->dims * 4, [&](void *dc, void *dv, int64_t cnt) -> int {
        launch_bq_decode(static_cast<uint64_t *>(dc), cnt, p->dims, static_cast<float *>(dv), p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(p->stream));
        return LB_OK;
    });
}

// ---- distances of stored rows -----------------------------------------------------------------------------------------
int lb_gpu_bq_hamming_batch(lb_gpu_bq *p, const uint64_t *qcode, int64_t row0, int64_t n, int32_t *results)
{
    if (!p || n < 0 || row0 < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!qcode || !results) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    Lease dq, dr;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        dq.reset(p->device, (size_t)p->W * 8);
        dr.reset(p->device, (size_t)n * 4);
        LB_HIP(hipMemcpyAsync(dq.p, qcode, (size_t)p->W * 8, hipMemcpyHostToDevice, p->stream));
        launch_bq_batch(p->d_codes.get(), p->W, dq.as<uint64_t>(), row0, n, dr.as<int32_t>(), p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpyAsync(results, dr.p, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
        LB_HIP(hipStreamSynchronize(p->stream));
        return LB_OK;
    });
}

int lb_gpu_bq_rerank_device(lb_gpu_bq *p, const uint64_t *d_qcode, const int64_t *d_rows, int64_t n, float *d_dist, float *d_score,
                            void *stream)
{
    if (!p || n < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!d_qcode || !d_rows || !d_dist) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        launch_bq_rerank(p->d_codes.get(), p->W, p->dims, p->n, d_qcode, d_rows, n, d_dist, d_score, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

int lb_gpu_bq_rerank(lb_gpu_bq *p, const uint64_t *qcode, const int64_t *rows, int64_t n, float *dist, float *score)
{
    if (!p || n < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!qcode || !rows || !dist) return LB_ERR_INVALID_ARG;
    Lease dq, drw, dd, ds;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        dq.reset(p->device, (size_t)p->W * 8);
        drw.reset(p->device, (size_t)n * 8);
        dd.reset(p->device, (size_t)n * 4);
        ds.reset(p->device, (size_t)n * 4);
        LB_HIP(hipMemcpy(dq.p, qcode, (size_t)p->W * 8, hipMemcpyHostToDevice));
        LB_HIP(hipMemcpy(drw.p, rows, (size_t)n * 8, hipMemcpyHostToDevice));
        const int rc = lb_gpu_bq_rerank_device(p, dq.as<uint64_t>(), drw.as<int64_t>(), n, dd.as<float>(), score ? ds.as<float>() : nullptr,
                                               nullptr);
        if (rc != LB_OK) return rc;
        LB_HIP(hipMemcpy(dist, dd.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (score) LB_HIP(hipMemcpy(score, ds.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- search ---------------------------------------------------------------------------------------------------------------
int lb_gpu_bq_search_device_ctx(lb_gpu_bq *p, int64_t nq, const float *d_queries, int k, float *d_dist, int64_t *d_labels, void *stream,
                                const lb_cancel *ctx)
{
    const int rc = knn_args(p, nq, d_queries, k, d_dist, d_labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    Lease dq, sc;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        dq.reset(p->device, (size_t)nq * p->W * 8);
        launch_bq_encode(d_queries, nq, p->dims, dq.as<uint64_t>(), s);
        return bq_search_codes_dev(p, nq, dq.as<uint64_t>(), k, d_dist, d_labels, s, ctx, sc);
    });
}

int lb_gpu_bq_search_ctx(lb_gpu_bq *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return host_search(p, nq, queries, false, k, dist, labels, ctx);
}

int lb_gpu_bq_search(lb_gpu_bq *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels)
{
    return host_search(p, nq, queries, false, k, dist, labels, nullptr);
}

int lb_gpu_bq_search_codes(lb_gpu_bq *p, int64_t nq, const uint64_t *qcodes, int k, float *dist, int64_t *labels)
{
    return host_search(p, nq, qcodes, true, k, dist, labels, nullptr);
}

} // extern "C"
