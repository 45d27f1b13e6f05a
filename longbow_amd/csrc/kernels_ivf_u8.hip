// kernels_ivf_u8.hip -- the list scan of an IVF-Flat handle whose rows are uint8 (ivf.hip; semantics in include/longbow_gpu.h,
// lb_gpu_ivf_new_u8).  The work decomposition is the list scans' (lb_list_scan.h): a workgroup takes a (query, probe slot) pair
// and walks 128-row tiles of that list, one lane owns one row.  A stage is the int8 scan's (kernels_ivf_i8.hip): 256 B of every
// row, gathered by row number in 16-byte pieces into an LDS tile whose row stride is 17 such pieces, the query's 256 B beside it
// and read wave-uniform, the next stage held in registers.  The arithmetic is the flat uint8 index's (kernels_u8.hip;
// lb_u8_exact.h), the reference's euclideanUint8Unrolled4x bit for bit -- but a list scan writes a key for EVERY row of a probed
// list, so it has no threshold to drop a pair beyond 2^24 against, and the exact integer path has to reach further than the
// total S <= 2^24.  It does so per chain: the reference sums four f32 chains over the residues i mod 4, every partial sum of
// chain j is an integer no larger than that chain's own exact sum S_j, so while every S_j <= 2^24 every add inside every chain is
// exact and the value is sqrt of ((f(S0) + f(S1)) + f(S2)) + f(S3) in f32 (u8_value_of_chains).  With D % 16 == 0 chain j is byte
// j of every 4-byte word, and v_dot4_u32_u8 of a row word masked to that byte against the query word is x_j q_j, against the row
// word itself x_j^2: S_j = n_j + qn_j - 2 a_j in exact uint32.  Two forms of the consume loop:
//   totals (D <= 258)  no pair can exceed 2^24 (258 * 65025 < 2^24): two accumulators, the int8 scan's instruction stream with
//                      unsigned dots, value u8_value_of_s(S)
//   chains (D > 258)   eight accumulators a_j, n_j; 4 ANDs and 8 dots per 4 row bytes.  Every pair for D <= 1032 has every
//                      S_j <= 2^24; beyond, a lane whose row has a chain past 2^24 evaluates the chain arithmetic itself from
//                      global memory (u8_chain_sum), divergent and uncoalesced on purpose: the rare path, with the loads of the
//                      next stage already in registers around it.
// The scan reads the uint8 queries of the batch themselves; the widened ones are the coarse index's.
// No FMA contraction here.
#include "lb_device.h"
#include "lb_ivf_u8.h"
#include "lb_list_scan.h"
#include "lb_select.h"
#include "lb_u8_exact.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

constexpr int U8L_ROWS = 128;          // rows per tile == threads per workgroup
constexpr int U8L_CK = 256;            // bytes per row per stage
constexpr int U8L_LD = U8L_CK + 16;    // LDS row stride (bytes): 17 16-byte slots, conflict-free ds_read_b128 by rows
constexpr int U8L_GEN_ROWS = 256;      // rows per tile of the generic form
constexpr int U8L_TOTALS_D = IVF_U8_TOTALS_D; // the largest D at which no pair exceeds 2^24: the totals form up to here

// one 4-byte word of the row against the query's: a[j] += x_j q_j, n[j] += x_j^2 for the word's four bytes j
__device__ __forceinline__ void u8l_chain_word(uint32_t w, uint32_t v, uint32_t (&a)[4], uint32_t (&n)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t m = w & (0xFFu << (8 * j));
        a[j] = __builtin_amdgcn_udot4(m, v, a[j], false);
        n[j] = __builtin_amdgcn_udot4(m, w, n[j], false);
    }
}

// Work = (query, probe slot, 128-row tile of that list), found and walked as lb_list_scan.h states.  A stage is [rows | query
// chunk] (128 x 272 + 256 + 16 = 35,088 B with the register-held prefetch of the next one, 4 workgroups per CU).  D % 16 == 0, X
// and Q 16-byte aligned.  CHAINS false: D <= 258.
template <bool CHAINS>
__global__ __launch_bounds__(U8L_ROWS) void ivf_scan_u8_kernel(IvfU8Scan s)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds_x[U8L_ROWS * U8L_LD];
    __shared__ __attribute__((aligned(16))) uint8_t lds_q[U8L_CK];
    __shared__ uint32_t lds_qn[4]; // the query's exact sum of q_i^2 per chain (totals form: all of it in [0])
    const IvfBatch &a = s.b;
    ListWork w;
    if (!ivf_list_work(a, U8L_ROWS, w)) return;
    const int tid = threadIdx.x;
    const int D = a.D;
    const int nchunks = (D + U8L_CK - 1) / U8L_CK;
    const uint32_t ntiles = (w.len + U8L_ROWS - 1) / U8L_ROWS;
    const uint8_t *q_src = s.Q + (int64_t)w.q * D;

    // the query's norms, once per workgroup
    uint32_t qn[4];
    {
        if (tid < 4) lds_qn[tid] = 0;
        __syncthreads();
        const uint32_t *q32 = reinterpret_cast<const uint32_t *>(q_src);
        uint32_t t[4] = {0, 0, 0, 0};
        for (int i = tid; i < (D >> 2); i += U8L_ROWS) {
            const uint32_t v = q32[i];
            if (CHAINS) {
#pragma unroll
                for (int j = 0; j < 4; j++) t[j] = __builtin_amdgcn_udot4(v & (0xFFu << (8 * j)), v, t[j], false);
            } else {
                t[0] = __builtin_amdgcn_udot4(v, v, t[0], false);
            }
        }
#pragma unroll
        for (int j = 0; j < (CHAINS ? 4 : 1); j++) atomicAdd(&lds_qn[j], t[j]);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; j++) qn[j] = lds_qn[j];
    }

    constexpr int PPR = U8L_CK / 16; // 16-byte pieces per row chunk == loads per thread per stage
    const bool q_loader = tid < PPR;
    u32x4 stg[PPR];
    u32x4 stq = {0, 0, 0, 0};
    uint32_t rid[PPR]; // the rows behind this thread's PPR staging slots of the tile being loaded
    auto load_stage = [&](uint32_t tile, int c) {
        const uint32_t trow0 = tile * U8L_ROWS;
        const int d0 = c * U8L_CK;
        if (q_loader) {
            int k = d0 + tid * 16;
            if (k > D - 16) k = D - 16;
            stq = *reinterpret_cast<const u32x4 *>(q_src + k);
        }
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < PPR; i++) {
                uint32_t pos = trow0 + ((uint32_t)(tid + U8L_ROWS * i) >> 4);
                if (pos >= w.len) pos = w.len - 1;
                rid[i] = w.rmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int p = (tid + U8L_ROWS * i) & (PPR - 1);
            int k = d0 + p * 16;
            if (k > D - 16) k = D - 16; // pieces past D are never consumed
            // (a plain load: other queries of the batch probe the same list and find it in L2 / MALL)
            stg[i] = *reinterpret_cast<const u32x4 *>(s.X + (int64_t)rid[i] * D + k);
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int ch = tid + U8L_ROWS * i;
            *reinterpret_cast<u32x4 *>(&lds_x[(ch >> 4) * U8L_LD + (ch & (PPR - 1)) * 16]) = stg[i];
        }
        if (q_loader) *reinterpret_cast<u32x4 *>(&lds_q[tid * 16]) = stq;
    };

    uint32_t acc[4] = {0, 0, 0, 0}; // sum x*q: per chain, or all of it in [0]
    uint32_t nx[4] = {0, 0, 0, 0};  // sum x*x, likewise
    float pend_dist = 0.f;
    uint32_t fin_tile = blockIdx.x; // the tile finish() is called for: the walk's, in its order
    auto consume = [&](int c) {
        if (c == 0) {
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] = nx[j] = 0;
        }
        const u32x4 *xr = reinterpret_cast<const u32x4 *>(&lds_x[tid * U8L_LD]);
        const u32x4 *qr = reinterpret_cast<const u32x4 *>(lds_q);
        const int d0 = c * U8L_CK;
        const int npieces = (min(D, d0 + U8L_CK) - d0) >> 4;
#pragma unroll 4
        for (int g = 0; g < npieces; g++) {
            const u32x4 x = xr[g];
            const u32x4 q = qr[g];
            if (CHAINS) {
                u8l_chain_word(x.x, q.x, acc, nx);
                u8l_chain_word(x.y, q.y, acc, nx);
                u8l_chain_word(x.z, q.z, acc, nx);
                u8l_chain_word(x.w, q.w, acc, nx);
            } else {
                acc[0] = __builtin_amdgcn_udot4(x.x, q.x, acc[0], false);
                acc[0] = __builtin_amdgcn_udot4(x.y, q.y, acc[0], false);
                acc[0] = __builtin_amdgcn_udot4(x.z, q.z, acc[0], false);
                acc[0] = __builtin_amdgcn_udot4(x.w, q.w, acc[0], false);
                nx[0] = __builtin_amdgcn_udot4(x.x, x.x, nx[0], false);
                nx[0] = __builtin_amdgcn_udot4(x.y, x.y, nx[0], false);
                nx[0] = __builtin_amdgcn_udot4(x.z, x.z, nx[0], false);
                nx[0] = __builtin_amdgcn_udot4(x.w, x.w, nx[0], false);
            }
        }
    };
    auto finish = [&]() {
        if (!CHAINS) { // S <= 258 * 65025 < 2^24
            pend_dist = u8_value_of_s(nx[0] + qn[0] - 2 * acc[0]);
            return;
        }
        // S_j <= 2048 * 65025 < 2^28, and 2 a_j < 2^29: exact in uint32
        uint32_t S[4];
#pragma unroll
        for (int j = 0; j < 4; j++) S[j] = nx[j] + qn[j] - 2 * acc[j];
        const uint32_t pos = fin_tile * U8L_ROWS + tid;
        fin_tile += gridDim.x;
        if (max(max(S[0], S[1]), max(S[2], S[3])) <= U8_EXACT_S) {
            pend_dist = u8_value_of_chains(S[0], S[1], S[2], S[3]);
        } else if (pos < w.len) { // (only for D > 1032; a lane past the list's end holds a copy of its last row and writes nothing)
            const float sum = u8_chain_sum<true>(s.X + (int64_t)w.rmap[pos] * D, q_src, D);
            pend_dist = (float)sqrt((double)sum);
        }
    };
    auto flush = [&](uint32_t tile) {
        const uint32_t pos = tile * U8L_ROWS + tid;
        if (pos < w.len) w.out[pos] = pack_entry(pend_dist, w.rmap[pos]);
    };
    walk_list_tiles(ntiles, nchunks, load_stage, write_stage, consume, finish, flush);
}

// Any other D or a misaligned base: one lane per row walks its row straight from global memory, in the chain arithmetic
// throughout (u8_pair_distance).
__global__ __launch_bounds__(U8L_GEN_ROWS) void ivf_scan_u8_generic_kernel(IvfU8Scan s)
{
    const IvfBatch &a = s.b;
    ListWork w;
    if (!ivf_list_work(a, U8L_GEN_ROWS, w)) return;
    const int D = a.D;
    const uint8_t *q = s.Q + (int64_t)w.q * D;
    for (uint64_t pos = (uint64_t)blockIdx.x * U8L_GEN_ROWS + threadIdx.x; pos < w.len; pos += (uint64_t)gridDim.x * U8L_GEN_ROWS) {
        const uint32_t row = w.rmap[pos];
        w.out[pos] = pack_entry(u8_pair_distance(s.X + (int64_t)row * D, q, D), row);
    }
}

void launch_ivf_scan_u8(const IvfU8Scan &a, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.b.nq * a.b.np;
    if (pairs <= 0 || maxlen <= 0) return;
    const bool staged = ivf_scan_u8_staged(a.b.D, a.X, a.Q);
    const dim3 grid = ivf_scan_grid(pairs, maxlen, staged ? U8L_ROWS : U8L_GEN_ROWS);
    if (!staged) hipLaunchKernelGGL(ivf_scan_u8_generic_kernel, grid, dim3(U8L_GEN_ROWS), 0, s, a);
    else if (a.b.D <= U8L_TOTALS_D) hipLaunchKernelGGL((ivf_scan_u8_kernel<false>), grid, dim3(U8L_ROWS), 0, s, a);
    else hipLaunchKernelGGL((ivf_scan_u8_kernel<true>), grid, dim3(U8L_ROWS), 0, s, a);
}

} // namespace lb
