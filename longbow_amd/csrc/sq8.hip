// sq8.hip -- host side of the lb_gpu_sq8_* entry points of include/longbow_gpu.h: store.SQ8Encoder
// (internal/store/scalar_quantization.go) and the exact k-NN over its codes by the integer distance.  The kernels are in
// kernels_sq8.hip.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_handle.h"

#include <atomic>
#include <vector>

using namespace lb;

struct lb_gpu_sq8 : FilteredHandle { // searches, reads and the codec share mu; adds, reserve, the bounds and the filter calls take it alone
    int stride = 0;
    DevBuf<uint8_t> d_codes;  // [capacity][stride], pad bytes zero
    DevBuf<int32_t> d_norms;  // [capacity]: sum of squares of each row, exact
    std::atomic<bool> trained{false};
    std::vector<float> h_min, h_max;
    DevBuf<float> d_par;      // [4][dims]: min, max, scale, invScale
    const float *dmin() const { return d_par.get(); }
    const float *dmax() const { return d_par.get() + dims; }
    const float *dscale() const { return d_par.get() + 2 * (size_t)dims; }
    const float *dinv() const { return d_par.get() + 3 * (size_t)dims; }
};

namespace {

constexpr int64_t kQueryBatch = 1024;                // queries per batch at most: bounds the histograms (8 MB) and the grid
constexpr int64_t kDistScratch = (int64_t)1 << 30;   // bytes of S a batch may hold

int untrained(lb_gpu_sq8 *p)
{
    p->set_error("config must be trained before creating encoder");
    return LB_ERR_INVALID_ARG;
}

void sq8_grow(lb_gpu_sq8 *p, int64_t need)
{
    if (need <= p->capacity) return;
    const int64_t cap = grow_capacity(p->capacity, need, (size_t)p->stride);
    DevBuf<uint8_t> nc;
    DevBuf<int32_t> nn;
    nc.alloc((size_t)cap * p->stride);
    nn.alloc((size_t)cap);
    if (p->n > 0) {
        LB_HIP(hipMemcpy(nc.get(), p->d_codes.get(), (size_t)p->n * p->stride, hipMemcpyDeviceToDevice));
        LB_HIP(hipMemcpy(nn.get(), p->d_norms.get(), (size_t)p->n * 4, hipMemcpyDeviceToDevice));
    }
    p->filter.grow(p->n, cap);
    p->d_codes = std::move(nc);
    p->d_norms = std::move(nn);
    p->capacity = cap;
}

// SQ8Config.Validate (scalar_quantization.go:44-49) and NewSQ8Encoder's scale / invScale (:75-79), in f32 on the host so
// that no device division enters; the caller holds the writer lock.  NaN bounds pass, as there.
int commit_bounds(lb_gpu_sq8 *p, const float *mn, const float *mx)
{
    const int D = p->dims;
    for (int i = 0; i < D; i++)
        if (mn[i] >= mx[i]) {
            p->set_error("min must be less than max for all dimensions");
            return LB_ERR_INVALID_ARG;
        }
    std::vector<float> par((size_t)4 * D);
    for (int i = 0; i < D; i++) {
        const volatile float range = mx[i] - mn[i];
        par[i] = mn[i];
        par[(size_t)D + i] = mx[i];
        par[(size_t)2 * D + i] = 255.0f / range;
        par[(size_t)3 * D + i] = range / 255.0f;
    }
    LB_HIP(hipSetDevice(p->device));
    p->d_par.ensure((size_t)4 * D);
    LB_HIP(hipMemcpy(p->d_par.get(), par.data(), (size_t)4 * D * 4, hipMemcpyHostToDevice));
    p->h_min.assign(mn, mn + D);
    p->h_max.assign(mx, mx + D);
    p->trained.store(true);
    return LB_OK;
}

int train_impl(lb_gpu_sq8 *p, int64_t n, const float *vectors, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) { p->set_error("no vectors provided for training"); return LB_ERR_INVALID_ARG; }
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (p->n > 0) { p->set_error("the bounds cannot change once rows are stored"); return LB_ERR_INVALID_ARG; }
    Lease st, part, dv;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        const int D = p->dims;
        const int64_t piece = on_device ? n : std::min(n, piece_rows(p->dims));
        st.reset(p->device, (size_t)2 * D * 4);
        part.reset(p->device, (size_t)2 * sq8_bounds_parts(piece) * D * 4);
        if (!on_device) dv.reset(p->device, (size_t)piece * D * 4);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            const float *X = vectors + (size_t)r0 * D;
            if (!on_device) {
                LB_HIP(hipMemcpyAsync(dv.p, X, (size_t)cnt * D * 4, hipMemcpyHostToDevice, s));
                X = dv.as<float>();
            }
            if (r0 == 0) launch_sq8_bounds_seed(X, D, st.as<float>(), s);
            launch_sq8_bounds_fold(X, cnt, D, part.as<float>(), st.as<float>(), s);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(s)); // the staging buffer is reused
        }
        std::vector<float> b((size_t)2 * D);
        LB_HIP(hipMemcpy(b.data(), st.p, (size_t)2 * D * 4, hipMemcpyDeviceToHost));
        float *mn = b.data(), *mx = b.data() + D;
        for (int i = 0; i < D; i++)
            if (mn[i] == mx[i]) { // scalar_quantization.go:121-125
                const volatile float e = mn[i] + 1e-7f;
                mx[i] = e;
            }
        return commit_bounds(p, mn, mx);
    });
}

// packed caller codes u8[n][dims] (host or device) -> d_dst u8[n][stride] with zero pads, on stream s; `tmp` stages them
void codes_in(lb_gpu_sq8 *p, const uint8_t *codes, bool on_device, int64_t n, uint8_t *d_dst, Lease &tmp, hipStream_t s)
{
    const size_t bytes = (size_t)n * p->dims;
    if (p->stride == p->dims) {
        LB_HIP(hipMemcpyAsync(d_dst, codes, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        return;
    }
    const uint8_t *src = codes;
    if (!on_device) {
        tmp.reset(p->device, bytes);
        LB_HIP(hipMemcpyAsync(tmp.p, codes, bytes, hipMemcpyHostToDevice, s));
        src = tmp.as<uint8_t>();
    }
    launch_sq8_restride(src, p->dims, d_dst, p->stride, p->dims, n, s);
}

// Exact k-NN of nq device-resident query codes u8[nq][stride] over the visible rows (S then holds a.n = n_visible positions per
// query, so a selective filter takes more queries per batch); the caller holds the reader lock, has made the device current
// and has checked the arguments.  ctx is polled before every launch.  The scratch is leased into the caller's `sc`, declared
// outside the caller's guard as lb_handle.h asks of every pooled buffer.
int sq8_search_codes_dev(lb_gpu_sq8 *p, int64_t nq, const uint8_t *d_Q, int k, float *d_dist, int64_t *d_labels, hipStream_t s,
                         const lb_cancel *ctx, Lease &sc)
{
    const RowView v = p->filter.view(p->n);
    Sq8Select a{};
    a.n = v.n;
    a.k = k;
    countsel_plan(a.n, SQ8_MAX_BLOCKS, &a.nblk, &a.tpb);
    // the largest batch whose distances fit the scratch, at least one query
    const int64_t nb = std::min(std::min(nq, kQueryBatch), std::max<int64_t>(1, kDistScratch / 4 / std::max<int64_t>(a.n, 1)));
    int32_t *d_S = nullptr, *d_qn = nullptr;
    auto layout = [&](Carve c) {
        a.S = d_S = c.take<int32_t>((size_t)nb * a.n * 4);
        d_qn = c.take<int32_t>((size_t)nb * 4);
        a.hist = c.take<uint32_t>((size_t)nb * SQ8_RADIX_BINS * 4);
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
        a.nq = (int)std::min(nb, nq - q0);
        if (a.n > 0) {
            const uint8_t *Q = d_Q + (size_t)q0 * p->stride;
            if (!go()) break;
            LB_HIP(hipMemsetAsync(a.hist, 0, (size_t)a.nq * SQ8_RADIX_BINS * 4, s)); // (every digit launch leaves it zero again)
            launch_sq8_norms(Q, a.nq, p->stride, d_qn, s);
            if (!go()) break;
            launch_sq8_dist(Sq8Dist{p->d_codes.get(), p->d_norms.get(), p->stride, 0, a.n, Q, d_qn, a.nq, d_S}, s, v.rowmap);
            for (int pass = 0; pass < 3 && !cancelled; pass++) {
                if (!go()) break;
                launch_sq8_hist(a, pass, s);
                if (!go()) break;
                launch_sq8_digit(a, pass, s);
            }
            if (cancelled || !go()) break;
            launch_sq8_count(a, s);
            if (!go()) break;
            launch_countsel_scan(a, s);
            if (!go()) break;
            launch_sq8_emit(a, s);
        }
        if (!go()) break;
        launch_countsel_finish(a, d_dist + (size_t)q0 * k, d_labels + (size_t)q0 * k, s, v.rowmap);
    }
    LB_LAUNCH_CHECK();
    LB_HIP(hipStreamSynchronize(s));
    return cancelled ? ctx_fail(p, cancelled) : LB_OK;
}

// knn_args with the untrained refusal of the entry points that encode their queries
int search_args(lb_gpu_sq8 *p, int64_t nq, const void *queries, int k, const void *dist, const void *labels, bool encodes,
                const lb_cancel *ctx)
{
    return knn_args(p, nq, queries, k, dist, labels, ctx, [&] { return encodes && !p->trained.load() ? untrained(p) : (int)LB_OK; });
}

// host queries (f32 rows, or packed codes when `coded`) -> search -> results back
int host_search(lb_gpu_sq8 *p, int64_t nq, const void *queries, bool coded, int k, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    const int rc = search_args(p, nq, queries, k, dist, labels, !coded, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    return host_knn(
        p, nq, (size_t)p->stride, k, dist, labels,
        [&](Lease &dq, Lease &dv, hipStream_t s) {
            if (coded) {
                codes_in(p, static_cast<const uint8_t *>(queries), false, nq, dq.as<uint8_t>(), dv, s);
                return;
            }
            dv.reset(p->device, (size_t)nq * p->dims * 4);
            LB_HIP(hipMemcpyAsync(dv.p, queries, (size_t)nq * p->dims * 4, hipMemcpyHostToDevice, s));
            launch_sq8_encode(dv.as<float>(), nq, p->dims, p->dmin(), p->dmax(), p->dscale(), dq.as<uint8_t>(), s);
        },
        [&](Lease &dq, float *d_dist, int64_t *d_labels, hipStream_t s, Lease &sc) {
            return sq8_search_codes_dev(p, nq, dq.as<uint8_t>(), k, d_dist, d_labels, s, ctx, sc);
        });
}

int add_codes_impl(lb_gpu_sq8 *p, int64_t n, const uint8_t *codes, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_fit(p, p->n, n)) return st;
    Lease tmp;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        sq8_grow(p, p->n + n);
        uint8_t *dst = p->d_codes.get() + (size_t)p->n * p->stride;
        codes_in(p, codes, on_device, n, dst, tmp, p->stream);
        launch_sq8_norms(dst, n, p->stride, p->d_norms.get() + p->n, p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(p->stream));
        p->filter.on_append(p->n, p->n + n, p->stream);
        p->n += n;
        return LB_OK;
    });
}

int add_vectors_impl(lb_gpu_sq8 *p, int64_t n, const float *vectors, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!p->trained.load()) return untrained(p);
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_fit(p, p->n, n)) return st;
    Lease dv;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        sq8_grow(p, p->n + n);
        const int64_t piece = on_device ? n : std::min(n, piece_rows(p->dims));
        if (!on_device) dv.reset(p->device, (size_t)piece * p->dims * 4);
        for (int64_t r0 = 0; r0 < n; r0 += piece) { // the rows become visible (p->n) only once all are encoded
            const int64_t cnt = std::min(piece, n - r0);
            const float *X = vectors + (size_t)r0 * p->dims;
            if (!on_device) {
                LB_HIP(hipMemcpyAsync(dv.p, X, (size_t)cnt * p->dims * 4, hipMemcpyHostToDevice, s));
                X = dv.as<float>();
            }
            uint8_t *dst = p->d_codes.get() + (size_t)(p->n + r0) * p->stride;
            launch_sq8_encode(X, cnt, p->dims, p->dmin(), p->dmax(), p->dscale(), dst, s);
            launch_sq8_norms(dst, cnt, p->stride, p->d_norms.get() + p->n + r0, s);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(s));
        }
        p->filter.on_append(p->n, p->n + n, s);
        p->n += n;
        return LB_OK;
    });
}

} // namespace

extern "C" {

lb_gpu_sq8 *lb_gpu_sq8_new(int device, int dims, int *out_status)
{
    return handle_new<lb_gpu_sq8>(device, dims, out_status, [](lb_gpu_sq8 *p) { p->stride = sq8_stride(p->dims); });
}

void lb_gpu_sq8_free(lb_gpu_sq8 *p) { handle_free(p); }
const char *lb_gpu_sq8_last_error(const lb_gpu_sq8 *p) { return handle_last_error(p); }
int lb_gpu_sq8_dims(const lb_gpu_sq8 *p) { return p ? p->dims : 0; }
int lb_gpu_sq8_trained(const lb_gpu_sq8 *p) { return p && p->trained.load() ? 1 : 0; }
int64_t lb_gpu_sq8_ntotal(const lb_gpu_sq8 *p) { return handle_ntotal(p); }
int lb_gpu_sq8_reserve(lb_gpu_sq8 *p, int64_t n_total) { return handle_reserve(p, n_total, sq8_grow); }

// ---- the row filter (lb_handle.h) ---------------------------------------------------------------------------------------
int64_t lb_gpu_sq8_nvisible(const lb_gpu_sq8 *p) { return filter_nvisible(p); }
int lb_gpu_sq8_set_filter(lb_gpu_sq8 *p, const uint8_t *mask, int64_t n) { return filter_set(p, mask, n); }
int lb_gpu_sq8_filter_int64(lb_gpu_sq8 *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                            int64_t validity_offset, int combine)
{
    return filter_column<int64_t>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_sq8_filter_float32(lb_gpu_sq8 *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                              int64_t validity_offset, int combine)
{
    return filter_column<float>(p, column, n, value, op, validity, validity_offset, combine);
}

// ---- bounds -----------------------------------------------------------------------------------------------------------
int lb_gpu_sq8_set_bounds(lb_gpu_sq8 *p, const float *min, const float *max)
{
    if (!p || !min || !max) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (p->n > 0) { p->set_error("the bounds cannot change once rows are stored"); return LB_ERR_INVALID_ARG; }
    return guard(p, nullptr, [&]() -> int { return commit_bounds(p, min, max); });
}

int lb_gpu_sq8_train(lb_gpu_sq8 *p, int64_t n, const float *vectors) { return train_impl(p, n, vectors, false); }
int lb_gpu_sq8_train_device(lb_gpu_sq8 *p, int64_t n, const float *d_vectors) { return train_impl(p, n, d_vectors, true); }

int lb_gpu_sq8_get_bounds(lb_gpu_sq8 *p, float *min, float *max)
{
    if (!p || !min || !max) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (!p->trained.load()) return untrained(p);
    std::copy(p->h_min.begin(), p->h_min.end(), min);
    std::copy(p->h_max.begin(), p->h_max.end(), max);
    return LB_OK;
}

// ---- adds and reads ---------------------------------------------------------------------------------------------------
int lb_gpu_sq8_add_codes(lb_gpu_sq8 *p, int64_t n, const uint8_t *codes) { return add_codes_impl(p, n, codes, false); }
int lb_gpu_sq8_add_codes_device(lb_gpu_sq8 *p, int64_t n, const uint8_t *d_codes) { return add_codes_impl(p, n, d_codes, true); }
int lb_gpu_sq8_add_vectors(lb_gpu_sq8 *p, int64_t n, const float *vectors) { return add_vectors_impl(p, n, vectors, false); }
int lb_gpu_sq8_add_vectors_device(lb_gpu_sq8 *p, int64_t n, const float *d_vectors) { return add_vectors_impl(p, n, d_vectors, true); }

int lb_gpu_sq8_get_codes(lb_gpu_sq8 *p, int64_t row0, int64_t n, uint8_t *codes)
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

// ---- Encode / Decode -----------------------------------------------------------------------------------------------
int lb_gpu_sq8_encode_device(lb_gpu_sq8 *p, int64_t n, const float *d_vectors, uint8_t *d_codes, void *stream)
{
    if (!p || n < 0 || (n > 0 && (!d_vectors || !d_codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!p->trained.load()) return untrained(p);
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    Lease tmp;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        if (p->stride == p->dims) {
            launch_sq8_encode(d_vectors, n, p->dims, p->dmin(), p->dmax(), p->dscale(), d_codes, s);
        } else { // the kernel writes whole 16-byte strides: pack them behind it
            const int64_t piece = std::min(n, piece_rows(p->dims));
            tmp.reset(p->device, (size_t)piece * p->stride);
            for (int64_t r0 = 0; r0 < n; r0 += piece) {
                const int64_t cnt = std::min(piece, n - r0);
                launch_sq8_encode(d_vectors + (size_t)r0 * p->dims, cnt, p->dims, p->dmin(), p->dmax(), p->dscale(), tmp.as<uint8_t>(), s);
                launch_sq8_restride(tmp.as<uint8_t>(), p->stride, d_codes + (size_t)r0 * p->dims, p->dims, p->dims, cnt, s);
            }
        }
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

int lb_gpu_sq8_encode(lb_gpu_sq8 *p, int64_t n, const float *vectors, uint8_t *codes)
{
    if (!p || n < 0 || (n > 0 && (!vectors || !codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!p->trained.load()) return untrained(p);
    return host_codec(p, n, vectors, (size_t)p->dims * 4, codes, (size_t)p->dims, [&](void *dv, void *dc, int64_t cnt) {
        return lb_gpu_sq8_encode_device(p, cnt, static_cast<float *>(dv), static_cast<uint8_t *>(dc), nullptr);
    });
}

int lb_gpu_sq8_decode(lb_gpu_sq8 *p, int64_t n, const uint8_t *codes, float *vectors)
{
    if (!p || n < 0 || (n > 0 && (!vectors || !codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!p->trained.load()) return untrained(p);
    std::shared_lock<std::shared_mutex> g(p->mu);
    return host_codec(p, n, codes, (size_t)p->dims, vectors, (size_t)p->dims * 4, [&](void *dc, void *dv, int64_t cnt) -> int {
        launch_sq8_decode(static_cast<uint8_t *>(dc), cnt, p->dims, p->dims, p->dmin(), p->dinv(), static_cast<float *>(dv), p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(p->stream));
        return LB_OK;
    });
}

// ---- distances of stored rows -----------------------------------------------------------------------------------------
int lb_gpu_sq8_distance_batch(lb_gpu_sq8 *p, const uint8_t *qcode, int64_t row0, int64_t n, int32_t *results)
{
    if (!p || n < 0 || row0 < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!qcode || !results) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    Lease dq, dr;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        dq.reset(p->device, (size_t)p->stride + 16); // the query at its stride, then its norm
        dr.reset(p->device, (size_t)n * 4);
        LB_HIP(hipMemsetAsync(dq.p, 0, (size_t)p->stride, s));
        LB_HIP(hipMemcpyAsync(dq.p, qcode, (size_t)p->dims, hipMemcpyHostToDevice, s));
        int32_t *d_qn = reinterpret_cast<int32_t *>(dq.as<char>() + p->stride);
        launch_sq8_norms(dq.as<uint8_t>(), 1, p->stride, d_qn, s);
        launch_sq8_dist(Sq8Dist{p->d_codes.get(), p->d_norms.get(), p->stride, row0, n, dq.as<uint8_t>(), d_qn, 1, dr.as<int32_t>()}, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpyAsync(results, dr.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

int lb_gpu_sq8_rerank_device(lb_gpu_sq8 *p, const uint8_t *d_qcode, const int64_t *d_rows, int64_t n, int32_t *d_s, float *d_euclid,
                             void *stream)
{
    if (!p || n < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!d_qcode || !d_rows || !d_s) return LB_ERR_INVALID_ARG;
    if (d_euclid && !p->trained.load()) return untrained(p);
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        launch_sq8_rerank(p->d_codes.get(), p->stride, p->dims, p->n, d_qcode, d_rows, n, d_euclid ? p->dmin() : nullptr,
                          d_euclid ? p->dinv() : nullptr, d_s, d_euclid, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

int lb_gpu_sq8_rerank(lb_gpu_sq8 *p, const uint8_t *qcode, const int64_t *rows, int64_t n, int32_t *s_out, float *euclid)
{
    if (!p || n < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!qcode || !rows || !s_out) return LB_ERR_INVALID_ARG;
    if (euclid && !p->trained.load()) return untrained(p);
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        Lease dq(p->device, (size_t)p->dims), drw(p->device, (size_t)n * 8), ds(p->device, (size_t)n * 4), de(p->device, (size_t)n * 4);
        LB_HIP(hipMemcpy(dq.p, qcode, (size_t)p->dims, hipMemcpyHostToDevice));
        LB_HIP(hipMemcpy(drw.p, rows, (size_t)n * 8, hipMemcpyHostToDevice));
        const int rc = lb_gpu_sq8_rerank_device(p, dq.as<uint8_t>(), drw.as<int64_t>(), n, ds.as<int32_t>(), euclid ? de.as<float>() : nullptr,
                                                nullptr);
        if (rc != LB_OK) return rc;
        LB_HIP(hipMemcpy(s_out, ds.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (euclid) LB_HIP(hipMemcpy(euclid, de.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- search ---------------------------------------------------------------------------------------------------------------
int lb_gpu_sq8_search_device_ctx(lb_gpu_sq8 *p, int64_t nq, const float *d_queries, int k, float *d_dist, int64_t *d_labels, void *stream,
                                 const lb_cancel *ctx)
{
    const int rc = search_args(p, nq, d_queries, k, d_dist, d_labels, true, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    Lease dq, sc;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        dq.reset(p->device, (size_t)nq * p->stride);
        launch_sq8_encode(d_queries, nq, p->dims, p->dmin(), p->dmax(), p->dscale(), dq.as<uint8_t>(), s);
        return sq8_search_codes_dev(p, nq, dq.as<uint8_t>(), k, d_dist, d_labels, s, ctx, sc);
    });
}

int lb_gpu_sq8_search_ctx(lb_gpu_sq8 *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return host_search(p, nq, queries, false, k, dist, labels, ctx);
}

int lb_gpu_sq8_search(lb_gpu_sq8 *p, int64_t nq, const float *queries, int k, float *dist, int64_t *labels)
{
    return host_search(p, nq, queries, false, k, dist, labels, nullptr);
}

int lb_gpu_sq8_search_codes(lb_gpu_sq8 *p, int64_t nq, const uint8_t *qcodes, int k, float *dist, int64_t *labels)
{
    return host_search(p, nq, qcodes, true, k, dist, labels, nullptr);
}

} // extern "C"
