// bq.hip -- host side of the lb_gpu_bq_* entry points of include/longbow_gpu.h: store.BQEncoder
// (internal/store/binary_quantization.go) and the exact Hamming k-NN over its codes.  The kernels are in kernels_bq.hip.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_host.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>

using namespace lb;

struct lb_gpu_bq {
    int device = 0, dims = 0, W = 0;
    std::shared_mutex mu; // searches and reads share it, adds and reserve take it alone
    DevBuf<uint64_t> d_codes;
    int64_t n = 0, capacity = 0;
    Stream stream;
    mutable std::mutex err_mu;
    std::string last_error;
    void set_error(const char *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        std::lock_guard<std::mutex> g(err_mu);
        try {
            last_error = buf;
        } catch (...) { // out of host memory: the status code still reaches the caller
        }
    }
};

namespace {

constexpr int64_t kMaxRows = 0x7fffffffll; // a key holds the row in 32 bits and the counts are u32
constexpr int64_t kQueryBatch = 1024;      // queries per pass of the selection: bounds its scratch (33 MB of histograms at W = 128)

int bq_fail(lb_gpu_bq *p, const HipErr &e)
{
    p->set_error("HIP error %d (%s) in %s", (int)e.e, hipGetErrorString(e.e), e.what);
    return e.e == hipErrorOutOfMemory ? LB_ERR_OOM : LB_ERR_HIP;
}

int bq_ctx_fail(lb_gpu_bq *p, int st)
{
    p->set_error(st == LB_ERR_CANCELLED ? "context canceled" : "context deadline exceeded");
    return st;
}

// The shell of an entry point: nothing but an lb_status leaves the library.  `s`, where given, is the stream the body
// enqueued on: it is drained before the answer, so that no kernel still runs on what the caller gets back.
template <class F> int bq_guard(lb_gpu_bq *p, hipStream_t s, F &&body) noexcept
{
    try {
        return body();
    } catch (const HipErr &e) {
        if (s) (void)hipStreamSynchronize(s);
        return bq_fail(p, e);
    } catch (const std::bad_alloc &) {
        if (s) (void)hipStreamSynchronize(s);
        p->set_error("out of host memory");
        return LB_ERR_OOM;
    } catch (...) {
        if (s) (void)hipStreamSynchronize(s);
        p->set_error("internal error (exception)");
        return LB_ERR_INTERNAL;
    }
}

// geometric growth, as pq_grow: beyond 1 GiB by at most 25 % + the request
void bq_grow(lb_gpu_bq *p, int64_t need)
{
    if (need <= p->capacity) return;
    int64_t cap = std::max<int64_t>(std::max<int64_t>(need, p->capacity * 2), 4096);
    if ((size_t)p->capacity * p->W * 8 > ((size_t)1 << 30)) cap = std::max<int64_t>(need, p->capacity + p->capacity / 4);
    DevBuf<uint64_t> nc;
    nc.alloc((size_t)cap * p->W);
    if (p->n > 0) LB_HIP(hipMemcpy(nc.get(), p->d_codes.get(), (size_t)p->n * p->W * 8, hipMemcpyDeviceToDevice));
    p->d_codes = std::move(nc);
    p->capacity = cap;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// rows of f32 per staging piece of the host-pointer codec calls (<= 64 Mi floats)
int64_t piece_rows(const lb_gpu_bq *p) { return std::max<int64_t>(1, ((int64_t)64 << 20) / p->dims); }

// Exact k-NN of nq device-resident query codes; the caller holds the reader lock, has made the device current and has checked
// the arguments.  ctx is polled before every launch.  The scratch is leased into the caller's `sc`, which like every pooled
// buffer of a search is declared outside the caller's bq_guard: an error drains the stream before any of them goes back to the
// pool, where a concurrent search could lease it.
int bq_search_codes_dev(lb_gpu_bq *p, int64_t nq, const uint64_t *d_Q, int k, float *d_dist, int64_t *d_labels, hipStream_t s,
                        const lb_cancel *ctx, Lease &sc)
{
    BqSearch a{};
    a.codes = p->d_codes.get();
    a.n = p->n;
    a.W = p->W;
    a.k = k;
    bq_search_plan(a.n, &a.nblk, &a.tpb);
    const size_t nbins = (size_t)64 * p->W + 1;
    const int64_t nb = std::min(nq, kQueryBatch);
    const size_t hist_b = up16((size_t)nb * nbins * 4), thr_b = up16((size_t)nb * 8), cnt_b = up16((size_t)nb * std::max(a.nblk, 1) * 8),
                 tot_b = up16((size_t)nb * 4), keys_b = (size_t)nb * k * 8;
    int cancelled = 0;
    sc.reset(p->device, hist_b + thr_b + cnt_b + tot_b + keys_b);
    char *base = sc.as<char>();
    a.hist = reinterpret_cast<uint32_t *>(base);
    a.thr = reinterpret_cast<uint32_t *>(base + hist_b);
    a.cnt = reinterpret_cast<uint32_t *>(base + hist_b + thr_b);
    a.tot = reinterpret_cast<uint32_t *>(base + hist_b + thr_b + cnt_b);
    a.keys = reinterpret_cast<uint64_t *>(base + hist_b + thr_b + cnt_b + tot_b);
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
            launch_bq_scan(a, s);
            if (!go()) break;
            launch_bq_emit(a, s);
        }
        if (!go()) break;
        launch_bq_finish(a, d_dist + (size_t)q0 * k, d_labels + (size_t)q0 * k, s);
    }
    LB_LAUNCH_CHECK();
    LB_HIP(hipStreamSynchronize(s));
    return cancelled ? bq_ctx_fail(p, cancelled) : LB_OK;
}

// INVALID_ARG, then UNSUPPORTED, then the context: what every search entry point answers before it touches the device
int search_args(lb_gpu_bq *p, int64_t nq, const void *queries, int k, const void *dist, const void *labels, const lb_cancel *ctx)
{
    if (!p || nq < 0 || k <= 0 || (nq > 0 && (!queries || !dist || !labels))) return LB_ERR_INVALID_ARG;
    if (k > LB_MAX_K) { p->set_error("k=%d exceeds the supported maximum %d", k, LB_MAX_K); return LB_ERR_UNSUPPORTED; }
    if (const int st = ctx_state(ctx)) return bq_ctx_fail(p, st);
    return LB_OK;
}

// host queries (f32 rows, or codes when `coded`) -> pooled device buffers -> search -> results back
int host_search(lb_gpu_bq *p, int64_t nq, const void *queries, bool coded, int k, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    const int rc = search_args(p, nq, queries, k, dist, labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(p->mu);
    Lease dq, dout, dv, sc;
    return bq_guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        const size_t qcb = (size_t)nq * p->W * 8, db = up16((size_t)nq * k * 4), lb = (size_t)nq * k * 8;
        dq.reset(p->device, qcb);
        dout.reset(p->device, db + lb);
        if (coded) {
            LB_HIP(hipMemcpyAsync(dq.p, queries, qcb, hipMemcpyHostToDevice, s));
        } else {
            dv.reset(p->device, (size_t)nq * p->dims * 4);
            LB_HIP(hipMemcpyAsync(dv.p, queries, (size_t)nq * p->dims * 4, hipMemcpyHostToDevice, s));
            launch_bq_encode(dv.as<float>(), nq, p->dims, dq.as<uint64_t>(), s);
        }
        float *d_dist = dout.as<float>();
        int64_t *d_labels = reinterpret_cast<int64_t *>(dout.as<char>() + db);
        const int src = bq_search_codes_dev(p, nq, dq.as<uint64_t>(), k, d_dist, d_labels, s, ctx, sc);
        if (src != LB_OK) return src;
        LB_HIP(hipMemcpy(dist, d_dist, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
        LB_HIP(hipMemcpy(labels, d_labels, lb, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

int add_codes_impl(lb_gpu_bq *p, int64_t n, const uint64_t *codes, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (n > kMaxRows - p->n) { p->set_error("2^31 or more codes per handle"); return LB_ERR_UNSUPPORTED; }
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        bq_grow(p, p->n + n);
        LB_HIP(hipMemcpy(p->d_codes.get() + (size_t)p->n * p->W, codes, (size_t)n * p->W * 8,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        p->n += n;
        return LB_OK;
    });
}

} // namespace

extern "C" {

lb_gpu_bq *lb_gpu_bq_new(int device, int dims, int *out_status)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    if (dims <= 0) { st(LB_ERR_INVALID_ARG); return nullptr; }
    if (dims > LB_MAX_DIM) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    if (!device_ok(device)) { st(LB_ERR_NO_DEVICE); return nullptr; }
    auto *p = new (std::nothrow) lb_gpu_bq();
    if (!p) { st(LB_ERR_OOM); return nullptr; }
    p->device = device;
    p->dims = dims;
    p->W = (dims + 63) / 64;
    try {
        LB_HIP(hipSetDevice(device));
        LB_HIP(hipStreamCreateWithFlags(&p->stream.h, hipStreamNonBlocking));
    } catch (const HipErr &e) {
        st(e.e == hipErrorOutOfMemory ? LB_ERR_OOM : LB_ERR_HIP);
        lb_gpu_bq_free(p);
        return nullptr;
    } catch (...) {
        st(LB_ERR_INTERNAL);
        lb_gpu_bq_free(p);
        return nullptr;
    }
    st(LB_OK);
    return p;
}

void lb_gpu_bq_free(lb_gpu_bq *p)
{
    if (!p) return;
    {
        std::unique_lock<std::shared_mutex> g(p->mu);
        (void)hipSetDevice(p->device);
        (void)hipDeviceSynchronize();
    }
    delete p;
}

const char *lb_gpu_bq_last_error(const lb_gpu_bq *p)
{
    if (!p) return "null handle";
    std::lock_guard<std::mutex> g(p->err_mu);
    return p->last_error.c_str();
}

int lb_gpu_bq_dims(const lb_gpu_bq *p) { return p ? p->dims : 0; }
int lb_gpu_bq_words(const lb_gpu_bq *p) { return p ? p->W : 0; }
int64_t lb_gpu_bq_ntotal(const lb_gpu_bq *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_bq *>(p)->mu);
    return p->n;
}

int lb_gpu_bq_reserve(lb_gpu_bq *p, int64_t n_total)
{
    if (!p || n_total < 0) return LB_ERR_INVALID_ARG;
    if (n_total > kMaxRows) { p->set_error("2^31 or more codes per handle"); return LB_ERR_UNSUPPORTED; }
    std::unique_lock<std::shared_mutex> g(p->mu);
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        bq_grow(p, n_total);
        return LB_OK;
    });
}

int lb_gpu_bq_add_codes(lb_gpu_bq *p, int64_t n, const uint64_t *codes) { return add_codes_impl(p, n, codes, false); }
int lb_gpu_bq_add_codes_device(lb_gpu_bq *p, int64_t n, const uint64_t *d_codes) { return add_codes_impl(p, n, d_codes, true); }

int lb_gpu_bq_get_codes(lb_gpu_bq *p, int64_t row0, int64_t n, uint64_t *codes)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (n > p->n || row0 > p->n - n) {
        p->set_error("rows [%lld, %lld) outside the %lld stored codes", (long long)row0, (long long)(row0 + n), (long long)p->n);
        return LB_ERR_INVALID_ARG;
    }
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        LB_HIP(hipMemcpy(codes, p->d_codes.get() + (size_t)row0 * p->W, (size_t)n * p->W * 8, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- Encode / Decode -----------------------------------------------------------------------------------------------
int lb_gpu_bq_encode_device(lb_gpu_bq *p, int64_t n, const float *d_vectors, uint64_t *d_codes, void *stream)
{
    if (!p || n < 0 || (n > 0 && (!d_vectors || !d_codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = stream ? (hipStream_t)stream : p->stream;
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
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        const int64_t piece = piece_rows(p);
        Lease dv(p->device, (size_t)std::min(n, piece) * p->dims * 4), dc(p->device, (size_t)std::min(n, piece) * p->W * 8);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            LB_HIP(hipMemcpy(dv.p, vectors + (size_t)r0 * p->dims, (size_t)cnt * p->dims * 4, hipMemcpyHostToDevice));
            const int rc = lb_gpu_bq_encode_device(p, cnt, dv.as<float>(), dc.as<uint64_t>(), nullptr);
            if (rc != LB_OK) return rc;
            LB_HIP(hipMemcpy(codes + (size_t)r0 * p->W, dc.p, (size_t)cnt * p->W * 8, hipMemcpyDeviceToHost));
        }
        return LB_OK;
    });
}

int lb_gpu_bq_add_vectors_device(lb_gpu_bq *p, int64_t n, const float *d_vectors)
{
    if (!p || n < 0 || (n > 0 && !d_vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (n > kMaxRows - p->n) { p->set_error("2^31 or more codes per handle"); return LB_ERR_UNSUPPORTED; }
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        bq_grow(p, p->n + n);
        launch_bq_encode(d_vectors, n, p->dims, p->d_codes.get() + (size_t)p->n * p->W, p->stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(p->stream));
        p->n += n;
        return LB_OK;
    });
}

int lb_gpu_bq_add_vectors(lb_gpu_bq *p, int64_t n, const float *vectors)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (n > kMaxRows - p->n) { p->set_error("2^31 or more codes per handle"); return LB_ERR_UNSUPPORTED; }
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        bq_grow(p, p->n + n);
        const int64_t piece = piece_rows(p);
        Lease dv(p->device, (size_t)std::min(n, piece) * p->dims * 4);
        for (int64_t r0 = 0; r0 < n; r0 += piece) { // the rows become visible (p->n) only once all are encoded
            const int64_t cnt = std::min(piece, n - r0);
            LB_HIP(hipMemcpy(dv.p, vectors + (size_t)r0 * p->dims, (size_t)cnt * p->dims * 4, hipMemcpyHostToDevice));
            launch_bq_encode(dv.as<float>(), cnt, p->dims, p->d_codes.get() + (size_t)(p->n + r0) * p->W, p->stream);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(p->stream));
        }
        p->n += n;
        return LB_OK;
    });
}

int lb_gpu_bq_decode(lb_gpu_bq *p, int64_t n, const uint64_t *codes, float *vectors)
{
    if (!p || n < 0 || (n > 0 && (!vectors || !codes))) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        const int64_t piece = piece_rows(p);
        Lease dv(p->device, (size_t)std::min(n, piece) * p->dims * 4), dc(p->device, (size_t)std::min(n, piece) * p->W * 8);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            LB_HIP(hipMemcpy(dc.p, codes + (size_t)r0 * p->W, (size_t)cnt * p->W * 8, hipMemcpyHostToDevice));
            launch_bq_decode(dc.as<uint64_t>(), cnt, p->dims, dv.as<float>(), p->stream);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(p->stream));
            LB_HIP(hipMemcpy(vectors + (size_t)r0 * p->dims, dv.p, (size_t)cnt * p->dims * 4, hipMemcpyDeviceToHost));
        }
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
    if (n > p->n || row0 > p->n - n) {
        p->set_error("rows [%lld, %lld) outside the %lld stored codes", (long long)row0, (long long)(row0 + n), (long long)p->n);
        return LB_ERR_INVALID_ARG;
    }
    Lease dq, dr;
    return bq_guard(p, p->stream, [&]() -> int {
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
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = stream ? (hipStream_t)stream : p->stream;
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
    return bq_guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        Lease dq(p->device, (size_t)p->W * 8), drw(p->device, (size_t)n * 8), dd(p->device, (size_t)n * 4), ds(p->device, (size_t)n * 4);
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
    const int rc = search_args(p, nq, d_queries, k, d_dist, d_labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    Lease dq, sc;
    return bq_guard(p, s, [&]() -> int {
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
