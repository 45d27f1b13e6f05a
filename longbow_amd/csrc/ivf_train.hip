// ivf_train.hip -- host side of lb_gpu_ivf_train*: pq.TrainKMeans (internal/pq/kmeans.go:64-151) for the coarse quantiser,
// nlist up to 65,536 centroids of whole rows.  It is lb_gpu_pq_train's contract with M = 1 (include/longbow_gpu.h) and shares
// its init, M-step and finish kernels; the E-step is kernels_ivf_train.hip's tile and the ordering is launch_ivf_sort.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_host.h"
#include "lb_ivf.h"

#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

using namespace lb;

namespace {

std::mutex g_timing_mu;
float g_timing_ms[3] = {0.f, 0.f, 0.f};

// everything that needs no device, in the order the header states; *vectors may be a host or a device pointer
int ivt_validate(int device, int dims, int nlist, int64_t n, const float *vectors, int max_iter, const int64_t *init_rows,
                 const float *centroids)
{
    if (!vectors || !centroids) return LB_ERR_INVALID_ARG;
    if (dims <= 0 || nlist <= 0 || n < nlist || max_iter < 0) return LB_ERR_INVALID_ARG; // "insufficient data for k-means: n < k"
    if (init_rows)
        for (int64_t i = 0; i < nlist; i++)
            if (init_rows[i] < 0 || init_rows[i] >= n) return LB_ERR_INVALID_ARG;
    if (nlist > IVF_MAX_NLIST || dims > LB_MAX_DIM) return LB_ERR_UNSUPPORTED;
    if (n > 0x7fffffffll) return LB_ERR_UNSUPPORTED; // rows are ordered as u32 / i32 words
    if (!device_ok(device)) return LB_ERR_NO_DEVICE;
    return LB_OK;
}

// the first K entries of a Fisher-Yates shuffle of [0, n): j = i + draw(seed, 0, i) mod (n - i), swap (i, j)
void ivt_draw_init_rows(uint64_t seed, int K, int64_t n, std::vector<int64_t> &rows)
{
    std::unordered_map<int64_t, int64_t> moved; // positions whose entry is no longer their own index
    auto at = [&](int64_t i) {
        auto f = moved.find(i);
        return f == moved.end() ? i : f->second;
    };
    for (int64_t i = 0; i < K; i++) {
        const int64_t j = i + (int64_t)(km_draw(seed, 0, (uint64_t)i) % (uint64_t)(n - i));
        const int64_t vi = at(i), vj = at(j);
        moved[j] = vi;
        rows[(size_t)i] = vj;
    }
}

// d_X: the n resident rows; arguments validated
int ivt_run(int device, int dims, int K, int64_t n, const float *d_X, int max_iter, uint64_t seed, const int64_t *init_rows,
            float *centroids, int32_t *iters_out, hipStream_t user_stream, const lb_cancel *ctx)
{
    const size_t ncent = (size_t)K * dims;
    std::vector<int64_t> rows((size_t)K);
    if (init_rows) std::memcpy(rows.data(), init_rows, (size_t)K * sizeof(int64_t));
    else ivt_draw_init_rows(seed, K, n, rows);
    if (const int st = ctx_state(ctx)) return st;
    try {
        LB_HIP(hipSetDevice(device));
        Stream own;
        if (!user_stream) LB_HIP(hipStreamCreateWithFlags(&own.h, hipStreamNonBlocking));
        hipStream_t s = user_stream ? user_stream : own.h;
        KmState st{};
        st.X = d_X; st.n = n; st.nchunks = 0; // (chunk_hist is lb_gpu_pq_train's ordering: not used here)
        st.D = dims; st.M = 1; st.K = K; st.sub = dims;
        DevBuf<float> d_cent;
        DevBuf<int32_t> d_assign;
        DevBuf<uint32_t> d_order, d_hist, d_words; // d_words: count [K], start = the sort's offsets [K + 1], changed, done, iters, bad
        DevBuf<int64_t> d_rows;
        PinnedBuf<uint32_t> h_state;
        d_cent.alloc(ncent);
        d_rows.alloc((size_t)K);
        d_words.alloc(2 * (size_t)K + 5);
        h_state.alloc(2);
        if (max_iter > 0) {
            d_assign.alloc((size_t)n);
            d_order.alloc((size_t)n);
            d_hist.alloc(ivf_sort_hist_words(n, K));
            LB_HIP(hipMemsetAsync(d_assign.get(), 0xff, (size_t)n * 4, s));
        }
        st.cent = d_cent.get(); st.assign = d_assign.get(); st.order = d_order.get(); st.chunk_hist = nullptr;
        st.count = d_words.get(); st.start = st.count + K; st.changed = st.start + K + 1; st.done = st.changed + 1;
        st.iters = reinterpret_cast<int32_t *>(st.done + 1); st.bad = st.done + 2;
        LB_HIP(hipMemsetAsync(d_words.get(), 0, d_words.count() * 4, s));
        LB_HIP(hipMemcpyAsync(d_rows.get(), rows.data(), (size_t)K * sizeof(int64_t), hipMemcpyHostToDevice, s));
        launch_km_init(st, d_rows.get(), s);
        EventH ev[4];
        const uint32_t thr = (uint32_t)(n / 1000 + 1); // kmeans.go:145
        // polled before every launch of an iteration: one E-step can be long at this shape
        auto cancelled = [&]() {
            const int cs = ctx_state(ctx);
            if (cs) (void)hipStreamSynchronize(s);
            return cs;
        };
        for (int it = 0; it < max_iter; it++) {
            if (const int cs = cancelled()) return cs;
            if (it == 0)
                for (auto &e : ev) LB_HIP(hipEventCreate(&e.h));
            if (it == 0) LB_HIP(hipEventRecord(ev[0], s));
            launch_ivt_estep(st, s);
            if (it == 0) LB_HIP(hipEventRecord(ev[1], s));
            if (const int cs = cancelled()) return cs;
            LB_HIP(launch_ivf_sort(reinterpret_cast<const uint32_t *>(st.assign), n, K, d_hist.get(), st.start, st.order, s));
            launch_ivt_counts(st.start, K, st.count, s);
            if (it == 0) LB_HIP(hipEventRecord(ev[2], s));
            if (const int cs = cancelled()) return cs;
            launch_km_mstep(st, seed, it, s);
            if (it == 0) LB_HIP(hipEventRecord(ev[3], s));
            if (const int cs = cancelled()) return cs;
            launch_km_finish(st, it, thr, h_state.get(), s);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(s)); // the one read-back of the iteration: h_state
            if (it == 0) {
                float ms[3] = {0.f, 0.f, 0.f};
                for (int i = 0; i < 3; i++)
                    if (hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) != hipSuccess) ms[i] = 0.f;
                std::lock_guard<std::mutex> g(g_timing_mu);
                std::memcpy(g_timing_ms, ms, sizeof ms);
            }
            if (h_state.get()[1]) return LB_ERR_INVALID_ARG; // the reference indexes counts[-1] here and panics
            if (h_state.get()[0] == 0) break;
        }
        std::vector<float> cent(ncent);
        int32_t iters = 0;
        LB_HIP(hipMemcpyAsync(cent.data(), st.cent, ncent * 4, hipMemcpyDeviceToHost, s));
        LB_HIP(hipMemcpyAsync(&iters, st.iters, 4, hipMemcpyDeviceToHost, s));
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        std::memcpy(centroids, cent.data(), ncent * 4);
        if (iters_out) *iters_out = iters;
    } catch (const HipErr &e) {
        return e.e == hipErrorOutOfMemory ? LB_ERR_OOM : LB_ERR_HIP;
    } catch (const std::bad_alloc &) {
        return LB_ERR_OOM;
    }
    return LB_OK;
}

} // namespace

extern "C" {

int lb_gpu_ivf_train_device(int device, int dims, int nlist, int64_t n, const float *d_vectors, int max_iter, uint64_t seed,
                            const int64_t *init_rows, float *centroids, int32_t *iters_out, void *stream, const lb_cancel *ctx)
{
    const int rc = ivt_validate(device, dims, nlist, n, d_vectors, max_iter, init_rows, centroids);
    if (rc != LB_OK) return rc;
    return ivt_run(device, dims, nlist, n, d_vectors, max_iter, seed, init_rows, centroids, iters_out, (hipStream_t)stream, ctx);
}

int lb_gpu_ivf_train(int device, int dims, int nlist, int64_t n, const float *vectors, int max_iter, uint64_t seed,
                     const int64_t *init_rows, float *centroids, int32_t *iters_out, const lb_cancel *ctx)
{
    const int rc = ivt_validate(device, dims, nlist, n, vectors, max_iter, init_rows, centroids);
    if (rc != LB_OK) return rc;
    DevBuf<float> d_X; // all rows stay resident for the iterations
    try {
        LB_HIP(hipSetDevice(device));
        d_X.alloc((size_t)n * dims);
        LB_HIP(hipMemcpy(d_X.get(), vectors, (size_t)n * dims * 4, hipMemcpyHostToDevice));
    } catch (const HipErr &e) {
        return e.e == hipErrorOutOfMemory ? LB_ERR_OOM : LB_ERR_HIP;
    }
    return ivt_run(device, dims, nlist, n, d_X.get(), max_iter, seed, init_rows, centroids, iters_out, nullptr, ctx);
}

int lb_gpu_ivf_train_last_timing(float ms[3])
{
    if (!ms) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(g_timing_mu);
    std::memcpy(ms, g_timing_ms, sizeof g_timing_ms);
    return LB_OK;
}

} // extern "C"
