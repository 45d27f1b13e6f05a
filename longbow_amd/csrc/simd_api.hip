// simd_api.hip -- the entry points of include/longbow_gpu.h that take a device, not a handle: the simd batch interface (lb_simd_*),
// merge, RRF, fill and the clock probe, with their small kernels and the process's buffer pool; and the candidate re-rank of an
// index, which stages through that pool as they do.  Their bodies run inside guard_device() / guard() (lb_handle.h).
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_host.h"
#include "lb_index.h"

#include <algorithm>
#include <cfloat>
#include <cstring>

using namespace lb;

namespace {

// one wave per CU spins for `ticks` of the constant 100 MHz counter and adds (shader cycles, ticks) to out[0 .. 1]
__global__ void clock_probe_kernel(unsigned long long *out, unsigned long long ticks)
{
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) {
        __builtin_amdgcn_s_sleep(8);
        r1 = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], c1 - c0);
        atomicAdd(&out[1], r1 - r0);
    }
}

__global__ void fill_empty_kernel(float *dist, int64_t *lab, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        dist[i] = FLT_MAX;
        lab[i] = -1;
    }
}
} // namespace
namespace lb {
// the canonical "no result" block: label -1 / distance FLT_MAX (also what comm.hip ships for a failed shard)
void launch_fill_empty(float *dist, int64_t *lab, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dist, lab, n);
}
} // namespace lb
namespace {

// candidate rows (int64 positions) -> u32 row map for the mapped scan; rows outside the corpus read row 0
// and are overwritten afterwards
__global__ void rerank_map_kernel(const int64_t *rows, int64_t n, int64_t ntotal, uint32_t *map)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int64_t r = rows[i];
        map[i] = (r >= 0 && r < ntotal) ? (uint32_t)r : 0u;
    }
}
// Score = 1/(1+d) (parallel_search.go:360); invalid rows: MaxFloat32 / 0
__global__ void rerank_score_kernel(const int64_t *rows, int64_t n, int64_t ntotal, float *dist, float *score)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int64_t r = rows[i];
        const bool ok = r >= 0 && r < ntotal;
        const float d = ok ? dist[i] : FLT_MAX;
        dist[i] = d;
        if (score) score[i] = ok ? __fdiv_rn(1.0f, 1.0f + d) : 0.f;
    }
}

} // namespace

namespace lb {
BufPool &buf_pool()
{
    static BufPool *pool = new BufPool(); // leaked on purpose: must outlive every handle at process exit
    return *pool;
}
} // namespace lb

// The shell of the handle-less calls: the device made current, then the body inside guard_device().  `stream` is what the body
// enqueues on (the caller's, or the null stream): an error drains it before the leases declared around the call return.
template <class Body> static int on_device(int device, void *stream, Body &&body)
{
    if (!device_ok(device)) return LB_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    return guard_device(s ? s : hipStreamLegacy, [&]() -> int {
        LB_HIP(hipSetDevice(device));
        return body(s);
    });
}
// one launch on the caller's stream, checked and drained
template <class Launch> static int launch_on_device(int device, void *stream, Launch &&launch)
{
    return on_device(device, stream, [&](hipStream_t s) -> int {
        launch(s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
}

template <typename T>
static int match_host(int device, const T *src, int64_t n, T value, int op, uint8_t *dst)
{
    if (n < 0 || op < 0 || op > 5) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!src || !dst) return LB_ERR_INVALID_ARG;
    Lease ds, dd;
    return on_device(device, nullptr, [&](hipStream_t s) -> int {
        ds.reset(device, (size_t)n * sizeof(T));
        dd.reset(device, (size_t)n);
        LB_HIP(hipMemcpy(ds.p, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice));
        if constexpr (sizeof(T) == 8) launch_match_int64(ds.as<int64_t>(), n, (int64_t)value, op, nullptr, 0, dd.as<uint8_t>(), 0, s);
        else launch_match_float32(ds.as<float>(), n, (float)value, op, nullptr, 0, dd.as<uint8_t>(), 0, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpy(dst, dd.p, (size_t)n, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

extern "C" {

int lb_simd_match_int64(int device, const int64_t *src, int64_t n, int64_t value, int op, uint8_t *dst)
{
    return match_host<int64_t>(device, src, n, value, op, dst);
}

int lb_simd_match_float32(int device, const float *src, int64_t n, float value, int op, uint8_t *dst)
{
    return match_host<float>(device, src, n, value, op, dst);
}

int lb_simd_and_bytes(int device, uint8_t *dst, const uint8_t *src, int64_t n)
{
    if (n < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!dst || !src) return LB_ERR_INVALID_ARG;
    Lease da, db;
    return on_device(device, nullptr, [&](hipStream_t s) -> int {
        da.reset(device, (size_t)n);
        db.reset(device, (size_t)n);
        LB_HIP(hipMemcpy(da.p, dst, (size_t)n, hipMemcpyHostToDevice));
        LB_HIP(hipMemcpy(db.p, src, (size_t)n, hipMemcpyHostToDevice));
        launch_and_bytes(da.as<uint8_t>(), db.as<uint8_t>(), n, s);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpy(dst, da.p, (size_t)n, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- candidate re-rank (processChunkInternal) ------------------------------------------
static int rerank_unsupported(lb_gpu_index *h)
{
    if (!h->f16_rows && !h->i8_rows) return LB_OK;
    h->set_error("re-rank reads float32 rows: not available on a %s index", h->i8_rows ? "int8" : "float16");
    return LB_ERR_UNSUPPORTED;
}

int lb_gpu_index_rerank_device(lb_gpu_index *h, const float *d_query, const int64_t *d_rows, int64_t n, int order,
                               float *d_dist, float *d_score, void *stream)
{
    if (!h || n < 0 || (order != -1 && order != LB_ORDER_SEQ && order != LB_ORDER_UNROLL4)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!d_query || !d_rows || !d_dist) return LB_ERR_INVALID_ARG;
    if (n > (int64_t)0x7fffffff) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(h->mu);
    if (const int rc = rerank_unsupported(h)) return rc;
    // a private stream per call when the caller gave none (the null stream would serialise callers)
    hipStream_t s = (hipStream_t)stream;
    std::unique_ptr<Workspace> w;
    if (!s) {
        const int rc = guard(h, nullptr, [&]() -> int {
            LB_HIP(hipSetDevice(h->device));
            int kc; uint32_t cap;
            cand_geometry(1, kc, cap);
            w = acquire_ws(h, 1, cap);
            return LB_OK;
        });
        if (rc != LB_OK) return rc;
        s = w->stream;
    }
    Lease map, qna;
    const int rc = guard(h, s, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        const int ord = order == -1 ? h->order.load() : order;
        map.reset(h->device, (size_t)n * sizeof(uint32_t));
        qna.reset(h->device, 16);
        const unsigned blocks = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(rerank_map_kernel, dim3(blocks), dim3(256), 0, s, d_rows, n, h->n, map.as<uint32_t>());
        if (h->n > 0) {
            if (h->metric == LB_METRIC_COSINE) launch_query_norms(ord, d_query, nullptr, 1, h->dim, qna.as<float>(), s);
            CandState cs{};
            launch_scan(h->metric, ord, /*raw_dot=*/false, h->d_X, 0, n, h->dim, d_query, nullptr, 1, qna.as<float>(), nullptr,
                        map.as<uint32_t>(), cs, false, d_dist, n, s);
        }
        hipLaunchKernelGGL(rerank_score_kernel, dim3(blocks), dim3(256), 0, s, d_rows, n, h->n, d_dist, d_score);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        return LB_OK;
    });
    if (w && rc == LB_OK) release_ws(h, std::move(w)); // (after an error the workspace is freed, not pooled)
    return rc;
}

int lb_gpu_index_rerank(lb_gpu_index *h, const float *query, const int64_t *rows, int64_t n, int order, float *dist,
                        float *score)
{
    if (!h || n < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!query || !rows || !dist) return LB_ERR_INVALID_ARG;
    if (const int rc = rerank_unsupported(h)) return rc;
    // [query | rows] up through one pinned block, [dist | score] back through another
    const size_t qb = up16((size_t)h->dim * 4), rb = (size_t)n * 8, ob = (size_t)n * 4;
    Lease hin, din, dout, hout;
    return guard(h, hipStreamLegacy, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        hin.reset(h->device, qb + rb, true);
        din.reset(h->device, qb + rb);
        dout.reset(h->device, 2 * ob);
        hout.reset(h->device, 2 * ob, true);
        std::memcpy(hin.p, query, (size_t)h->dim * 4);
        std::memcpy(hin.as<char>() + qb, rows, rb);
        LB_HIP(hipMemcpy(din.p, hin.p, qb + rb, hipMemcpyHostToDevice));
        const int rc = lb_gpu_index_rerank_device(h, din.as<float>(), reinterpret_cast<const int64_t *>(din.as<char>() + qb), n,
                                                  order, dout.as<float>(), dout.as<float>() + n, nullptr);
        if (rc != LB_OK) return rc;
        LB_HIP(hipMemcpy(hout.p, dout.p, 2 * ob, hipMemcpyDeviceToHost));
        std::memcpy(dist, hout.p, ob);
        if (score) std::memcpy(score, hout.as<char>() + ob, ob);
        return LB_OK;
    });
}

// ---- simd batch interface ---------------------------------------------------------
int lb_simd_distance_batch_flat_device(int device, int metric, int order, const float *d_query,
                                       const float *d_flat, int64_t n, int dims, float *d_results, void *stream)
{
    if (metric < 0 || metric > 2 || (order != 0 && order != 1) || n < 0 || dims < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK; // batch_operations.go:65-67
    if (!d_query || !d_flat || !d_results || dims == 0) return LB_ERR_INVALID_ARG;
    if (dims > LB_MAX_DIM) return LB_ERR_UNSUPPORTED;
    Lease qna;
    return launch_on_device(device, stream, [&](hipStream_t s) {
        qna.reset(device, 16);
        if (metric == LB_METRIC_COSINE) launch_query_norms(order, d_query, nullptr, 1, dims, qna.as<float>(), s);
        CandState cs{};
        launch_scan(metric, order, /*raw_dot=*/true, d_flat, 0, n, dims, d_query, nullptr, 1, qna.as<float>(), nullptr, nullptr,
                    cs, false, d_results, n, s);
    });
}

int lb_simd_distance_batch_flat(int device, int metric, int order, const float *query, const float *flat,
                                int64_t n, int dims, float *results)
{
    if (metric < 0 || metric > 2 || (order != 0 && order != 1) || n < 0 || dims < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    if (!query || !flat || !results || dims == 0) return LB_ERR_INVALID_ARG;
    Lease dq, dx, dr;
    return on_device(device, nullptr, [&](hipStream_t) -> int {
        dq.reset(device, (size_t)dims * 4);
        dx.reset(device, (size_t)n * dims * 4);
        dr.reset(device, (size_t)n * 4);
        LB_HIP(hipMemcpy(dq.p, query, (size_t)dims * 4, hipMemcpyHostToDevice));
        LB_HIP(hipMemcpy(dx.p, flat, (size_t)n * dims * 4, hipMemcpyHostToDevice));
        const int rc = lb_simd_distance_batch_flat_device(device, metric, order, dq.as<float>(), dx.as<float>(), n, dims,
                                                          dr.as<float>(), nullptr);
        if (rc != LB_OK) return rc;
        LB_HIP(hipMemcpy(results, dr.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// simd.EuclideanDistanceBatch / CosineDistanceBatch / DotProductBatch over [][]float32
// (internal/simd/batch_operations.go:29-60,131-157; per-vector rules in include/longbow_gpu.h)
int lb_simd_distance_batch(int device, int metric, int order, const float *query, int dims, const float *const *vectors,
                           const int *lens, int64_t n, float *results)
{
    if (metric < 0 || metric > 2 || (order != 0 && order != 1) || n < 0 || dims < 0) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK; // batch_operations.go:33-35,132-134
    if (!vectors || !lens || !results || (dims > 0 && !query)) return LB_ERR_INVALID_ARG;
    if (dims > LB_MAX_DIM) return LB_ERR_UNSUPPORTED;
    // which vectors are scored
    std::vector<int64_t> live;
    try {
        live.reserve((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const bool ok = vectors[i] != nullptr && lens[i] == dims;
            if (metric == LB_METRIC_EUCLIDEAN) {
                if (ok) live.push_back(i);
                else results[i] = FLT_MAX; // math.MaxFloat32 (batch_operations.go:39-42,51)
            } else {
                if (vectors[i] == nullptr) continue; // skipped: results[i] keeps the caller's value (simd.go:243-245,256-258)
                if (lens[i] != dims) break;          // the loop returns its error here and the wrapper swallows it (:140,155)
                live.push_back(i);
            }
        }
    } catch (...) {
        return LB_ERR_OOM;
    }
    const int64_t m = (int64_t)live.size();
    if (m == 0) return LB_OK;
    if (dims == 0) { // len 0: 0 (Euclidean, dot) / 1.0 (cosine)  (simd.go:131-163)
        for (int64_t i : live) results[i] = metric == LB_METRIC_COSINE ? 1.0f : 0.0f;
        return LB_OK;
    }
    const size_t row = (size_t)dims * 4;
    Lease hx, dq, dx, dr, hr;
    return on_device(device, nullptr, [&](hipStream_t) -> int {
        hx.reset(device, (size_t)m * row, true);
        dq.reset(device, row);
        dx.reset(device, (size_t)m * row);
        dr.reset(device, (size_t)m * 4);
        hr.reset(device, (size_t)m * 4, true);
        for (int64_t j = 0; j < m; j++) std::memcpy(hx.as<char>() + (size_t)j * row, vectors[live[(size_t)j]], row);
        LB_HIP(hipMemcpy(dq.p, query, row, hipMemcpyHostToDevice));
        LB_HIP(hipMemcpy(dx.p, hx.p, (size_t)m * row, hipMemcpyHostToDevice));
        const int rc = lb_simd_distance_batch_flat_device(device, metric, order, dq.as<float>(), dx.as<float>(), m, dims,
                                                          dr.as<float>(), nullptr);
        if (rc != LB_OK) return rc;
        LB_HIP(hipMemcpy(hr.p, dr.p, (size_t)m * 4, hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < m; j++) results[live[(size_t)j]] = hr.as<float>()[j];
        return LB_OK;
    });
}

// ---- merge / fill -----------------------------------------------------------------
int lb_gpu_merge_topk_device(int device, int nshards, int64_t nq, int k, const float *d_dist_in,
                             const int64_t *d_labels_in, float *d_dist_out, int64_t *d_labels_out, void *stream)
{
    if (nshards <= 0 || nq < 0 || k <= 0 || (int64_t)nshards * k > 16384) return LB_ERR_INVALID_ARG;
    if (nq == 0) return LB_OK;
    if (!d_dist_in || !d_labels_in || !d_dist_out || !d_labels_out) return LB_ERR_INVALID_ARG;
    return launch_on_device(device, stream, [&](hipStream_t s) {
        launch_merge_topk(nshards, nq, k, d_dist_in, d_labels_in, nq * k, nq * k, d_dist_out, d_labels_out, s);
    });
}

int lb_gpu_merge_topk_packed_device(int device, int nshards, int64_t nq, int k, const void *d_packed,
                                    float *d_dist_out, int64_t *d_labels_out, void *stream)
{
    if (nshards <= 0 || nq < 0 || k <= 0 || (int64_t)nshards * k > 16384) return LB_ERR_INVALID_ARG;
    if (nq == 0) return LB_OK;
    if (!d_packed || !d_dist_out || !d_labels_out) return LB_ERR_INVALID_ARG;
    // per shard: nq*k int64 labels followed by nq*k f32 distances (padded to 8 bytes)
    const int64_t nk = nq * k;
    const int64_t block_bytes = nk * 8 + ((nk * 4 + 7) / 8) * 8;
    const char *base = reinterpret_cast<const char *>(d_packed);
    return launch_on_device(device, stream, [&](hipStream_t s) {
        launch_merge_topk(nshards, nq, k, reinterpret_cast<const float *>(base + nk * 8), reinterpret_cast<const int64_t *>(base),
                          block_bytes / 4, block_bytes / 8, d_dist_out, d_labels_out, s);
    });
}

int lb_gpu_rrf_fuse_device(int device, int64_t nq, int kd, const int64_t *d_dense_ids, int ks,
                           const int64_t *d_sparse_ids, int k, int limit, int64_t *d_out_ids,
                           float *d_out_scores, void *stream)
{
    if (nq < 0 || kd < 0 || ks < 0 || limit <= 0 || kd + ks > 8192) return LB_ERR_INVALID_ARG;
    if (nq == 0) return LB_OK;
    if ((kd > 0 && !d_dense_ids) || (ks > 0 && !d_sparse_ids) || !d_out_ids || !d_out_scores) return LB_ERR_INVALID_ARG;
    return launch_on_device(device, stream, [&](hipStream_t s) {
        launch_rrf(nq, kd, d_dense_ids, ks, d_sparse_ids, k <= 0 ? 60 : k, limit, d_out_ids, d_out_scores, s);
    });
}

int lb_gpu_rrf_fuse(int device, int64_t nq, int kd, const int64_t *dense_ids, int ks, const int64_t *sparse_ids,
                    int k, int limit, int64_t *out_ids, float *out_scores)
{
    if (nq < 0 || kd < 0 || ks < 0 || limit <= 0 || kd + ks > 8192) return LB_ERR_INVALID_ARG;
    if (nq == 0) return LB_OK;
    if ((kd > 0 && !dense_ids) || (ks > 0 && !sparse_ids) || !out_ids || !out_scores) return LB_ERR_INVALID_ARG;
    Lease dd, ds, dout, dsc;
    return on_device(device, nullptr, [&](hipStream_t) -> int {
        dd.reset(device, (size_t)nq * std::max(kd, 1) * 8);
        ds.reset(device, (size_t)nq * std::max(ks, 1) * 8);
        dout.reset(device, (size_t)nq * limit * 8);
        dsc.reset(device, (size_t)nq * limit * 4);
        if (kd > 0) LB_HIP(hipMemcpy(dd.p, dense_ids, (size_t)nq * kd * 8, hipMemcpyHostToDevice));
        if (ks > 0) LB_HIP(hipMemcpy(ds.p, sparse_ids, (size_t)nq * ks * 8, hipMemcpyHostToDevice));
        const int rc = lb_gpu_rrf_fuse_device(device, nq, kd, dd.as<int64_t>(), ks, ds.as<int64_t>(), k, limit,
                                              dout.as<int64_t>(), dsc.as<float>(), nullptr);
        if (rc != LB_OK) return rc;
        LB_HIP(hipMemcpy(out_ids, dout.p, (size_t)nq * limit * 8, hipMemcpyDeviceToHost));
        LB_HIP(hipMemcpy(out_scores, dsc.p, (size_t)nq * limit * 4, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

int lb_gpu_fill_uniform_device(int device, float *d_dst, int64_t n, uint64_t seed, int64_t offset, void *stream)
{
    if (n < 0 || (n > 0 && !d_dst)) return LB_ERR_INVALID_ARG;
    return launch_on_device(device, stream, [&](hipStream_t s) { launch_fill_uniform(d_dst, n, seed, offset, s); });
}

int lb_gpu_fill_uniform_rows_device(int device, float *d_dst, const int64_t *d_ids, int64_t nrows, int dim, uint64_t seed,
                                    void *stream)
{
    if (nrows < 0 || dim <= 0 || (nrows > 0 && (!d_dst || !d_ids))) return LB_ERR_INVALID_ARG;
    return launch_on_device(device, stream, [&](hipStream_t s) { launch_fill_uniform_rows(d_dst, d_ids, nrows, dim, seed, s); });
}

double lb_gpu_shader_clock_mhz(int device, int spin_us)
{
    if (spin_us <= 0 || spin_us > 1000000) return -(double)LB_ERR_INVALID_ARG;
    double mhz = 0.0;
    Lease d, hbuf;
    const int rc = on_device(device, nullptr, [&](hipStream_t s) -> int {
        int cus = 0;
        LB_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        if (cus <= 0) cus = 1;
        d.reset(device, 2 * sizeof(unsigned long long));
        hbuf.reset(device, 2 * sizeof(unsigned long long), true);
        LB_HIP(hipMemset(d.p, 0, 2 * sizeof(unsigned long long)));
        hipLaunchKernelGGL(clock_probe_kernel, dim3((unsigned)cus), dim3(64), 0, s, d.as<unsigned long long>(),
                           (unsigned long long)spin_us * 100ull);
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpy(hbuf.p, d.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        const unsigned long long *v = hbuf.as<unsigned long long>();
        if (v[1] == 0) return LB_ERR_INTERNAL;
        mhz = 100.0 * (double)v[0] / (double)v[1];
        return LB_OK;
    });
    return rc == LB_OK ? mhz : -(double)rc;
}

int lb_gpu_fill_codes_device(int device, uint8_t *d_dst, int64_t n, uint64_t seed, int64_t offset, void *stream)
{
    if (n < 0 || (n > 0 && !d_dst)) return LB_ERR_INVALID_ARG;
    return launch_on_device(device, stream, [&](hipStream_t s) { launch_fill_codes(d_dst, n, seed, offset, s); });
}

} // extern "C"
