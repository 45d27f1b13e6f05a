// kernels_ivf_i8.hip -- the list scan of an IVF-Flat handle whose rows are int8 (ivf.hip; semantics in include/longbow_gpu.h,
// lb_gpu_ivf_new_i8).  The work decomposition is the list scans' (lb_list_scan.h): a workgroup takes a (query, probe slot) pair
// and walks 128-row tiles of that list, one lane owns one row.  A stage holds 256 B of every row, the fp16 kernel's
// (kernels_ivf_f16.hip) bytes of a row and so its bytes in flight, gathered by row number in 16-byte pieces into an LDS tile
// whose row stride is 17 such pieces.  The arithmetic is the flat int8 index's (kernels_i8.hip): x.q by v_dot4_i32_i8 in exact int32; for L2 |x|^2 comes
// from the same instruction over the row's own bytes in the same loop, so the handle keeps no norm array and an add has no pass
// over the rows, and S = |x|^2 + |q|^2 - 2 x.q is the exact integer sum of (x_i - q_i)^2, rounded once to f32.  The scan reads the
// int8 queries of the batch themselves; the widened ones are the coarse index's.
// No FMA contraction here.
#include "lb_device.h"
#include "lb_i8_exact.h"
#include "lb_ivf_i8.h"
#include "lb_list_scan.h"
#include "lb_select.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int I8L_ROWS = 128;          // rows per tile == threads per workgroup
constexpr int I8L_CK = 256;            // bytes per row per stage
constexpr int I8L_LD = I8L_CK + 16;    // LDS row stride (bytes): 17 16-byte slots, conflict-free ds_read_b128 by rows
constexpr int I8L_GEN_ROWS = 256;      // rows per tile of the generic form

// Work = (query, probe slot, 128-row tile of that list), found and walked as lb_list_scan.h states.  A stage is [rows | query
// chunk] (128 x 272 + 256 + 4 = 35,076 B with the register-held prefetch of the next one, 4 workgroups per CU).  D % 16 == 0, X
// and Q 16-byte aligned; dot: D <= 1024, so that the total is the exact integer the four chains of dotInt8Unrolled4x sum to.
template <int METRIC>
__global__ __launch_bounds__(I8L_ROWS) void ivf_scan_i8_kernel(IvfI8Scan s)
{
    __shared__ __attribute__((aligned(16))) int8_t lds_x[I8L_ROWS * I8L_LD];
    __shared__ __attribute__((aligned(16))) int8_t lds_q[I8L_CK];
    __shared__ int lds_qn;
    const IvfBatch &a = s.b;
    ListWork w;
    if (!ivf_list_work(a, I8L_ROWS, w)) return;
    const int tid = threadIdx.x;
    const int D = a.D;
    const int nchunks = (D + I8L_CK - 1) / I8L_CK;
    const uint32_t ntiles = (w.len + I8L_ROWS - 1) / I8L_ROWS;
    const int8_t *q_src = s.Q + (int64_t)w.q * D;

    // the query's exact |q|^2 (L2), once per workgroup
    int qn = 0;
    if (METRIC == METRIC_L2) {
        if (tid == 0) lds_qn = 0;
        __syncthreads();
        const int *q32 = reinterpret_cast<const int *>(q_src);
        int t = 0;
        for (int i = tid; i < (D >> 2); i += I8L_ROWS) {
            const int v = q32[i];
            t = __builtin_amdgcn_sdot4(v, v, t, false);
        }
        atomicAdd(&lds_qn, t);
        __syncthreads();
        qn = lds_qn;
    }

    constexpr int PPR = I8L_CK / 16; // 16-byte pieces per row chunk == loads per thread per stage
    const bool q_loader = tid < PPR;
    i32x4 stg[PPR];
    i32x4 stq = {0, 0, 0, 0};
    uint32_t rid[PPR]; // the rows behind this thread's PPR staging slots of the tile being loaded
    auto load_stage = [&](uint32_t tile, int c) {
        const uint32_t trow0 = tile * I8L_ROWS;
        const int d0 = c * I8L_CK;
        if (q_loader) {
            int k = d0 + tid * 16;
            if (k > D - 16) k = D - 16;
            stq = *reinterpret_cast<const i32x4 *>(q_src + k);
        }
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < PPR; i++) {
                uint32_t pos = trow0 + ((uint32_t)(tid + I8L_ROWS * i) >> 4);
                if (pos >= w.len) pos = w.len - 1;
                rid[i] = w.rmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int p = (tid + I8L_ROWS * i) & (PPR - 1);
            int k = d0 + p * 16;
            if (k > D - 16) k = D - 16; // pieces past D are never consumed
            // (a plain load: other queries of the batch probe the same list and find it in L2 / MALL)
            stg[i] = *reinterpret_cast<const i32x4 *>(s.X + (int64_t)rid[i] * D + k);
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int ch = tid + I8L_ROWS * i;
            *reinterpret_cast<i32x4 *>(&lds_x[(ch >> 4) * I8L_LD + (ch & (PPR - 1)) * 16]) = stg[i];
        }
        if (q_loader) *reinterpret_cast<i32x4 *>(&lds_q[tid * 16]) = stq;
    };

    int acc = 0; // sum x*q
    int nx = 0;  // L2: sum x*x
    float pend_dist = 0.f;
    auto consume = [&](int c) {
        if (c == 0) {
            acc = 0;
            nx = 0;
        }
        const i32x4 *xr = reinterpret_cast<const i32x4 *>(&lds_x[tid * I8L_LD]);
        const i32x4 *qr = reinterpret_cast<const i32x4 *>(lds_q);
        const int d0 = c * I8L_CK;
        const int npieces = (min(D, d0 + I8L_CK) - d0) >> 4;
#pragma unroll 4
        for (int g = 0; g < npieces; g++) {
            const i32x4 x = xr[g];
            const i32x4 q = qr[g];
            acc = __builtin_amdgcn_sdot4(x.x, q.x, acc, false);
            acc = __builtin_amdgcn_sdot4(x.y, q.y, acc, false);
            acc = __builtin_amdgcn_sdot4(x.z, q.z, acc, false);
            acc = __builtin_amdgcn_sdot4(x.w, q.w, acc, false);
            if (METRIC == METRIC_L2) {
                nx = __builtin_amdgcn_sdot4(x.x, x.x, nx, false);
                nx = __builtin_amdgcn_sdot4(x.y, x.y, nx, false);
                nx = __builtin_amdgcn_sdot4(x.z, x.z, nx, false);
                nx = __builtin_amdgcn_sdot4(x.w, x.w, nx, false);
            }
        }
    };
    auto finish = [&]() {
        // L2: S <= 8192 * 65025 < 2^31, converted once to f32, sqrt correctly rounded; dot: |x.q| <= 2^24, exact
        if (METRIC == METRIC_L2) pend_dist = (float)sqrt((double)(float)(nx + qn - 2 * acc));
        else pend_dist = -(float)acc;
    };
    auto flush = [&](uint32_t tile) {
        const uint32_t pos = tile * I8L_ROWS + tid;
        if (pos < w.len) w.out[pos] = pack_entry(pend_dist, w.rmap[pos]);
    };
    walk_list_tiles(ntiles, nchunks, load_stage, write_stage, consume, finish, flush);
}

// Any other D, a misaligned base, or dot beyond 1024 dimensions: one lane per row walks its row straight from global memory, in
// the arithmetic of i8_pair_distance.
template <int METRIC>
__global__ __launch_bounds__(I8L_GEN_ROWS) void ivf_scan_i8_generic_kernel(IvfI8Scan s)
{
    const IvfBatch &a = s.b;
    ListWork w;
    if (!ivf_list_work(a, I8L_GEN_ROWS, w)) return;
    const int D = a.D;
    const int8_t *q = s.Q + (int64_t)w.q * D;
    for (uint64_t pos = (uint64_t)blockIdx.x * I8L_GEN_ROWS + threadIdx.x; pos < w.len; pos += (uint64_t)gridDim.x * I8L_GEN_ROWS) {
        const uint32_t row = w.rmap[pos];
        w.out[pos] = pack_entry(i8_pair_distance<METRIC>(s.X + (int64_t)row * D, q, D), row);
    }
}

template <int METRIC>
static void launch_ivf_scan_i8_m(const IvfI8Scan &a, bool staged, dim3 grid, hipStream_t s)
{
    if (staged) hipLaunchKernelGGL((ivf_scan_i8_kernel<METRIC>), grid, dim3(I8L_ROWS), 0, s, a);
    else hipLaunchKernelGGL((ivf_scan_i8_generic_kernel<METRIC>), grid, dim3(I8L_GEN_ROWS), 0, s, a);
}

void launch_ivf_scan_i8(int metric, const IvfI8Scan &a, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.b.nq * a.b.np;
    if (pairs <= 0 || maxlen <= 0) return;
    const bool staged = a.b.D % 16 == 0 && (metric == METRIC_L2 || a.b.D <= 1024) &&
                        ((reinterpret_cast<uintptr_t>(a.X) | reinterpret_cast<uintptr_t>(a.Q)) & 15) == 0;
    const dim3 grid = ivf_scan_grid(pairs, maxlen, staged ? I8L_ROWS : I8L_GEN_ROWS);
    if (metric == METRIC_L2) launch_ivf_scan_i8_m<METRIC_L2>(a, staged, grid, s);
    else launch_ivf_scan_i8_m<METRIC_DOT>(a, staged, grid, s);
}

} // namespace lb
