// kernels_ivf_f16.hip -- the list scan of an IVF-Flat handle whose rows are float16 (ivf.hip; semantics in include/longbow_gpu.h,
// lb_gpu_ivf_new_f16).  The work decomposition is the list scans' (lb_list_scan.h): a workgroup takes a (query, probe slot)
// pair and walks 128-row tiles of that list, one lane owns one row and carries that row's f32 accumulator chain(s) across D in the
// reference's order (lb_exact.h).  The staging differs from ivf_scan_kernel's (kernels_ivf.hip): a stage holds 128 elements of
// every row, which is the f32 kernel's 256 B of a row and so its bytes in flight, and the rows stay fp16 in LDS; a lane widens
// its row's elements to f32 as it reads them, which is exact, so the chains see what they see over the widened rows and the
// keys are the f32 scan's bit for bit.
// No FMA contraction here.
#include "lb_device.h"
#include "lb_exact.h"
#include "lb_ivf_f16.h"
#include "lb_list_scan.h"
#include "lb_select.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

constexpr int IH_ROWS = 128;       // rows per tile == threads per workgroup
constexpr int IH_DK = 128;         // halves per row per stage: 256 B
constexpr int IH_LD = IH_DK + 8;   // padded LDS row stride (halves): 68 dwords, the f32 tile's, conflict-free ds_read_b128
constexpr int IH_GEN_ROWS = 256;   // rows per tile of the generic form

// Work = (query, probe slot, 128-row tile of that list), found and walked as lb_list_scan.h states.  A stage is [rows fp16 |
// query chunk f32] (128 x 272 + 128 x 4 = 35,328 B with the register-held prefetch of the next one, 4 workgroups per CU).
// D % 8 == 0, X and Q 16-byte aligned.
template <int METRIC, int ORDER>
__global__ __launch_bounds__(IH_ROWS) void ivf_scan_f16_kernel(IvfF16Scan s)
{
    __shared__ __attribute__((aligned(16))) _Float16 lds_x[IH_ROWS * IH_LD];
    __shared__ __attribute__((aligned(16))) float lds_q[IH_DK];
    const IvfBatch &a = s.b;
    ListWork w;
    if (!ivf_list_work(a, IH_ROWS, w)) return;
    const int tid = threadIdx.x;
    const int D = a.D;
    const int nchunks = (D + IH_DK - 1) / IH_DK;
    const uint32_t ntiles = (w.len + IH_ROWS - 1) / IH_ROWS;
    const float *q_src = a.Q + (int64_t)w.q * D;
    const float na = METRIC == METRIC_COS ? a.qna[w.q] : 0.f;

    constexpr int PPR = IH_DK / 8; // 16-byte pieces per row chunk == loads per thread per stage
    const bool q_loader = tid < IH_DK / 4;
    f16x8 stg[PPR];
    f32x4 stq = {0.f, 0.f, 0.f, 0.f};
    uint32_t rid[PPR]; // the rows behind this thread's PPR staging slots of the tile being loaded
    auto load_stage = [&](uint32_t tile, int c) {
        const uint32_t trow0 = tile * IH_ROWS;
        const int d0 = c * IH_DK;
        if (q_loader) {
            int k = d0 + tid * 4;
            if (k > D - 4) k = D - 4;
            stq = *reinterpret_cast<const f32x4 *>(q_src + k);
        }
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < PPR; i++) {
                uint32_t pos = trow0 + ((uint32_t)(tid + IH_ROWS * i) >> 4);
                if (pos >= w.len) pos = w.len - 1;
                rid[i] = w.rmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int p = (tid + IH_ROWS * i) & (PPR - 1);
            int k = d0 + p * 8;
            if (k > D - 8) k = D - 8; // pieces past D are never consumed
            // (a plain load: other queries of the batch probe the same list and find it in L2 / MALL)
            stg[i] = *reinterpret_cast<const f16x8 *>(s.X + (int64_t)rid[i] * D + k);
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int ch = tid + IH_ROWS * i;
            *reinterpret_cast<f16x8 *>(&lds_x[(ch >> 4) * IH_LD + (ch & (PPR - 1)) * 8]) = stg[i];
        }
        if (q_loader) *reinterpret_cast<f32x4 *>(&lds_q[tid * 4]) = stq;
    };

    Acc<ORDER> acc; // L2: sum (q-x)^2 ; cos/dot: sum q*x
    Acc<ORDER> nb;  // cos: sum x*x
    float pend_dist = 0.f;
    auto consume = [&](int c) {
        if (c == 0) {
            acc.zero();
            nb.zero();
        }
        const _Float16 *xr = &lds_x[tid * IH_LD];
        const int d0 = c * IH_DK;
        const int npieces = (min(D, d0 + IH_DK) - d0) >> 3;
#pragma unroll 2
        for (int g = 0; g < npieces; g++) {
            const f16x8 xh = *reinterpret_cast<const f16x8 *>(&xr[g * 8]);
            const f32x4 lo = {(float)xh[0], (float)xh[1], (float)xh[2], (float)xh[3]};
            const f32x4 hi = {(float)xh[4], (float)xh[5], (float)xh[6], (float)xh[7]};
            if (METRIC == METRIC_COS) nb.add4_sq(lo);
            acc.template add4_pair<METRIC>(*reinterpret_cast<const f32x4 *>(&lds_q[g * 8]), lo);
            if (METRIC == METRIC_COS) nb.add4_sq(hi);
            acc.template add4_pair<METRIC>(*reinterpret_cast<const f32x4 *>(&lds_q[g * 8 + 4]), hi);
        }
    };
    auto finish = [&]() { pend_dist = exact_distance<METRIC>(acc.total(), nb.total(), na, D, false); };
    auto flush = [&](uint32_t tile) {
        const uint32_t pos = tile * IH_ROWS + tid;
        if (pos < w.len) w.out[pos] = pack_entry(pend_dist, w.rmap[pos]);
    };
    walk_list_tiles(ntiles, nchunks, load_stage, write_stage, consume, finish, flush);
}

// D % 8 != 0 or a misaligned base: one lane per row walks its row straight from global memory.  Same arithmetic.
template <int METRIC, int ORDER>
__global__ __launch_bounds__(IH_GEN_ROWS) void ivf_scan_f16_generic_kernel(IvfF16Scan s)
{
    const IvfBatch &a = s.b;
    ListWork w;
    if (!ivf_list_work(a, IH_GEN_ROWS, w)) return;
    const int D = a.D;
    const float *q = a.Q + (int64_t)w.q * D;
    const float na = METRIC == METRIC_COS ? a.qna[w.q] : 0.f;
    for (uint64_t pos = (uint64_t)blockIdx.x * IH_GEN_ROWS + threadIdx.x; pos < w.len; pos += (uint64_t)gridDim.x * IH_GEN_ROWS) {
        const uint32_t row = w.rmap[pos];
        float t, nbt;
        exact_pair_sums<METRIC, ORDER, _Float16>(s.X + (int64_t)row * D, q, D, t, nbt);
        w.out[pos] = pack_entry(exact_distance<METRIC>(t, nbt, na, D, false), row);
    }
}

void launch_ivf_scan_f16(int metric, int order, const IvfF16Scan &a, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.b.nq * a.b.np;
    if (pairs <= 0 || maxlen <= 0) return;
    const bool staged = a.b.D % 8 == 0 && ((reinterpret_cast<uintptr_t>(a.X) | reinterpret_cast<uintptr_t>(a.b.Q)) & 15) == 0;
    const dim3 grid = ivf_scan_grid(pairs, maxlen, staged ? IH_ROWS : IH_GEN_ROWS);
    with_metric_order(metric, order, [&](auto m, auto o) {
        if (staged) hipLaunchKernelGGL((ivf_scan_f16_kernel<decltype(m)::value, decltype(o)::value>), grid, dim3(IH_ROWS), 0, s, a);
        else hipLaunchKernelGGL((ivf_scan_f16_generic_kernel<decltype(m)::value, decltype(o)::value>), grid, dim3(IH_GEN_ROWS), 0, s, a);
    });
}

} // namespace lb
