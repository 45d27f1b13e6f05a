// pq_train.hip -- host side of lb_gpu_pq_train*: pq.(*PQEncoder).Train (internal/pq/encoder.go:38-73), i.e.
// pq.TrainKMeans (internal/pq/kmeans.go:64-151) per subspace, with the random draws restated as documented counter-based
// ones (include/longbow_gpu.h).  The kernels are in kernels_pq_train.hip; the result is the persistence.go blob that
// lb_gpu_pq_new reads.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_host.h"

#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

using namespace lb;

namespace {

std::mutex g_timing_mu;
float g_timing_ms[3] = {0.f, 0.f, 0.f};

void wr_u32le(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// everything that needs no device, in the order the header states; *vectors may be a host or a device pointer
int train_validate(int device, int dims, int M, int K, int64_t n, const float *vectors, int max_iter, const int64_t *init_rows,
                   const uint8_t *blob, size_t blob_len)
{
    if (!vectors || !blob) return LB_ERR_INVALID_ARG;
    if (M <= 0 || dims <= 0 || dims % M != 0) return LB_ERR_INVALID_ARG; // "dimension must be divisible by M"
    if (K < 0 || n < 0 || n < K) return LB_ERR_INVALID_ARG;               // "insufficient data for k-means: n < k"
    if (max_iter < 0) return LB_ERR_INVALID_ARG;
    if (blob_len != 12 + (size_t)M * (size_t)K * (size_t)(dims / M) * 4) return LB_ERR_INVALID_ARG;
    if (init_rows)
        for (int64_t i = 0; i < (int64_t)M * K; i++)
            if (init_rows[i] < 0 || init_rows[i] >= n) return LB_ERR_INVALID_ARG;
    if (K < 1 || K > 256 || dims > LB_MAX_DIM) return LB_ERR_UNSUPPORTED;
    if (n > 0x7fffffffll) return LB_ERR_UNSUPPORTED; // rows are ordered as u32 / i32 words
    if (!device_ok(device)) return LB_ERR_NO_DEVICE;
    return LB_OK;
}

// the first K entries of a Fisher-Yates shuffle of [0, n): j = i + draw(seed, m, i) mod (n - i), swap (i, j)
void draw_init_rows(uint64_t seed, int M, int K, int64_t n, std::vector<int64_t> &rows)
{
    for (int m = 0; m < M; m++) {
        std::unordered_map<int64_t, int64_t> moved; // positions whose entry is no longer their own index
        auto at = [&](int64_t i) {
            auto f = moved.find(i);
            return f == moved.end() ? i : f->second;
        };
        for (int64_t i = 0; i < K; i++) {
            const int64_t j = i + (int64_t)(km_draw(seed, (uint64_t)m, (uint64_t)i) % (uint64_t)(n - i));
            const int64_t vi = at(i), vj = at(j);
            moved[j] = vi;
            rows[(size_t)m * K + i] = vj;
        }
    }
}

// d_X: the n resident rows; arguments validated
int train_run(int device, int dims, int M, int K, int64_t n, const float *d_X, int max_iter, uint64_t seed,
              const int64_t *init_rows, uint8_t *blob, int32_t *iters_out, hipStream_t user_stream, const lb_cancel *ctx)
{
    const int sub = dims / M;
    const size_t MK = (size_t)M * K, ncent = MK * sub;
    std::vector<int64_t> rows(MK);
    if (init_rows) std::memcpy(rows.data(), init_rows, MK * sizeof(int64_t));
    else draw_init_rows(seed, M, K, n, rows);
    if (const int st = ctx_state(ctx)) return st;
    try {
        LB_HIP(hipSetDevice(device));
        Stream own;
        if (!user_stream) LB_HIP(hipStreamCreateWithFlags(&own.h, hipStreamNonBlocking));
        hipStream_t s = user_stream ? user_stream : own.h;
        KmState st{};
        st.X = d_X; st.n = n; st.nchunks = (n + KM_CHUNK - 1) / KM_CHUNK;
        st.D = dims; st.M = M; st.K = K; st.sub = sub;
        const size_t Mn = (size_t)M * (size_t)n, nhist = (size_t)M * (size_t)st.nchunks * K;
        DevBuf<float> d_cent;
        DevBuf<int32_t> d_assign;
        DevBuf<uint32_t> d_order, d_hist, d_words; // d_words: count, start [M*K each], changed, done, iters [M each], bad
        DevBuf<int64_t> d_rows;
        PinnedBuf<uint32_t> h_state;
        d_cent.alloc(ncent);
        d_rows.alloc(MK);
        d_words.alloc(2 * MK + 3 * (size_t)M + 1);
        h_state.alloc(2);
        if (max_iter > 0) {
            d_assign.alloc(Mn);
            d_order.alloc(Mn);
            d_hist.alloc(nhist);
            LB_HIP(hipMemsetAsync(d_assign.get(), 0xff, Mn * 4, s));
            LB_HIP(hipMemsetAsync(d_hist.get(), 0, nhist * 4, s));
        }
        st.cent = d_cent.get(); st.assign = d_assign.get(); st.order = d_order.get(); st.chunk_hist = d_hist.get();
        st.count = d_words.get(); st.start = st.count + MK; st.changed = st.start + MK; st.done = st.changed + M;
        st.iters = reinterpret_cast<int32_t *>(st.done + M); st.bad = st.done + 2 * (size_t)M;
        LB_HIP(hipMemsetAsync(d_words.get(), 0, d_words.count() * 4, s));
        LB_HIP(hipMemcpyAsync(d_rows.get(), rows.data(), MK * sizeof(int64_t), hipMemcpyHostToDevice, s));
        launch_km_init(st, d_rows.get(), s);
        EventH ev[4];
        const uint32_t thr = (uint32_t)(n / 1000 + 1); // kmeans.go:145
        for (int it = 0; it < max_iter; it++) {
            if (const int cs = ctx_state(ctx)) { // polled once per iteration
                (void)hipStreamSynchronize(s);
                return cs;
            }
            if (it == 0)
                for (auto &e : ev) LB_HIP(hipEventCreate(&e.h));
            if (it == 0) LB_HIP(hipEventRecord(ev[0], s));
            launch_km_estep(st, s);
            if (it == 0) LB_HIP(hipEventRecord(ev[1], s));
            launch_km_order(st, s);
            if (it == 0) LB_HIP(hipEventRecord(ev[2], s));
            launch_km_mstep(st, seed, it, s);
            if (it == 0) LB_HIP(hipEventRecord(ev[3], s));
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
        std::vector<int32_t> iters((size_t)M);
        LB_HIP(hipMemcpyAsync(cent.data(), st.cent, ncent * 4, hipMemcpyDeviceToHost, s));
        LB_HIP(hipMemcpyAsync(iters.data(), st.iters, (size_t)M * 4, hipMemcpyDeviceToHost, s));
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        // persistence.go:9-35 (f32 little-endian on the wire == host layout on this platform)
        wr_u32le(blob, (uint32_t)dims);
        wr_u32le(blob + 4, (uint32_t)M);
        wr_u32le(blob + 8, (uint32_t)K);
        std::memcpy(blob + 12, cent.data(), ncent * 4);
        if (iters_out) std::memcpy(iters_out, iters.data(), (size_t)M * 4);
    } catch (const HipErr &e) {
        return e.e == hipErrorOutOfMemory ? LB_ERR_OOM : LB_ERR_HIP;
    } catch (const std::bad_alloc &) {
        return LB_ERR_OOM;
    }
    return LB_OK;
}

} // namespace

extern "C" {

size_t lb_gpu_pq_blob_bytes(int dims, int M, int K)
{
    if (dims <= 0 || M <= 0 || K <= 0 || dims % M != 0) return 0;
    return 12 + (size_t)M * (size_t)K * (size_t)(dims / M) * 4;
}

int lb_gpu_pq_train_device(int device, int dims, int M, int K, int64_t n, const float *d_vectors, int max_iter, uint64_t seed,
                           const int64_t *init_rows, uint8_t *blob, size_t blob_len, int32_t *iters_out, void *stream,
                           const lb_cancel *ctx)
{
    const int rc = train_validate(device, dims, M, K, n, d_vectors, max_iter, init_rows, blob, blob_len);
    if (rc != LB_OK) return rc;
    return train_run(device, dims, M, K, n, d_vectors, max_iter, seed, init_rows, blob, iters_out, (hipStream_t)stream, ctx);
}

int lb_gpu_pq_train(int device, int dims, int M, int K, int64_t n, const float *vectors, int max_iter, uint64_t seed,
                    const int64_t *init_rows, uint8_t *blob, size_t blob_len, int32_t *iters_out, const lb_cancel *ctx)
{
    const int rc = train_validate(device, dims, M, K, n, vectors, max_iter, init_rows, blob, blob_len);
    if (rc != LB_OK) return rc;
    DevBuf<float> d_X; // all rows stay resident for the iterations
    try {
        LB_HIP(hipSetDevice(device));
        d_X.alloc((size_t)n * dims);
        LB_HIP(hipMemcpy(d_X.get(), vectors, (size_t)n * dims * 4, hipMemcpyHostToDevice));
    } catch (const HipErr &e) {
        return e.e == hipErrorOutOfMemory ? LB_ERR_OOM : LB_ERR_HIP;
    }
    return train_run(device, dims, M, K, n, d_X.get(), max_iter, seed, init_rows, blob, iters_out, nullptr, ctx);
}

int lb_gpu_pq_train_last_timing(float ms[3])
{
    if (!ms) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(g_timing_mu);
    std::memcpy(ms, g_timing_ms, sizeof g_timing_ms);
    return LB_OK;
}

} // extern "C"
