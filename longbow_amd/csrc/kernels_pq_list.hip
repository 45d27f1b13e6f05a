// kernels_pq_list.hip -- the ADC search of kernels_pq.hip / kernels_pq2.hip under a row filter.
//
// With a filter the handle holds the ascending list of its visible rows (lb_handle.h: RowFilter) and a search walks the
// list's POSITIONS instead of the rows: the sampled threshold scores evenly spaced positions, the exact scan and the byte-table
// prefilter take positions [pos_begin, pos_end).  Each lane owns one position, reads its row id (the 64 ids of a wave's tile
// are one coalesced 256-B load) and gathers that row's M code bytes.  The arithmetic is the unfiltered kernels':
//     exact     f32 sum of table[j*256 + code_j] in j order, float(sqrt(double(sum))), pack_entry(dist, row)
//     prefilter integer sum S of the byte table's entries, the row survives iff (int)S <= s_tau
// and the entries and candidates carry CORPUS rows: the list is ascending, so (distance, row) orders as (distance, position)
// does, and launch_select, launch_adc_exact_candidates and the emit follow unchanged.  Only the boot chunk's slot index is a
// position (pos - pos_begin).
//
// Row fetch: the aligned forms (M % 16 == 0, 16-B aligned codes) load a row as M/16 per-lane 16-B global loads straight into
// registers; the prefilter keeps the loads of its NEXT position in flight under the gathers of the current one.  (The
// alternative, a per-lane global_load_lds gather into a lane-linear staging slot read back by its lane, was built and measured
// 5 to 10 % slower at 10 % and 50 % visible and level at 1 %: LABNOTES R14.1.)  The generic
// forms (any M, or misaligned codes) read single bytes.  No load leaves [codes, codes + n*M): a lane past the end of the list
// reads neither the list nor the codes.
//
// These are separate kernels, not a mapped mode of the streaming ones: sharing a body with the unmapped kernels costs those
// registers (LABNOTES: the BQ filter work), and the kernels an unfiltered search launches stay what they were.
#include "lb_device.h"
#include "lb_exact.h"

#pragma clang fp contract(off)

namespace lb {

constexpr int ADC_LIST_THREADS = ADC_LIST_WAVES * 64;
constexpr int ADC_LIST_MAX_BLOCKS = 256; // one workgroup per CU holds the table once (as the streaming kernels)

// ---- sampled threshold ----------------------------------------------------------------------------------------------
// adc_sample_kernel over the list: sample i is position i * n_vis / count
template <bool VEC16>
__global__ __launch_bounds__(ADC_LIST_THREADS) void adc_list_sample_kernel(const float *table, int M, const uint8_t *codes,
                                                                           const uint32_t *rowmap, int64_t n_vis, uint32_t count,
                                                                           uint64_t *out)
{
    extern __shared__ __attribute__((aligned(16))) float tab[];
    for (int i = threadIdx.x; i < M * 256; i += ADC_LIST_THREADS) tab[i] = table[i];
    __syncthreads();
    for (uint32_t i = blockIdx.x * ADC_LIST_THREADS + threadIdx.x; i < count; i += gridDim.x * ADC_LIST_THREADS) {
        const uint64_t pos = ((uint64_t)i * (uint64_t)n_vis) / count; // i < count, n_vis < 2^31: pos < n_vis
        const uint32_t row = rowmap[pos];
        const float sum = adc_row_sum<VEC16>(tab, codes + (int64_t)row * M, M);
        out[i] = pack_entry(adc_distance(sum), row);
    }
}

void launch_adc_list_sample(const float *table, int M, const uint8_t *codes, const uint32_t *rowmap, int64_t n_vis,
                            uint32_t count, uint64_t *out, hipStream_t s)
{
    if (count == 0 || n_vis <= 0) return;
    const bool vec = (M % 16 == 0) && ((reinterpret_cast<uintptr_t>(codes) & 15) == 0);
    const size_t shmem = (size_t)M * 256 * sizeof(float);
    uint32_t blocks = (count + ADC_LIST_THREADS - 1) / ADC_LIST_THREADS;
    if (blocks > (uint32_t)ADC_LIST_MAX_BLOCKS) blocks = ADC_LIST_MAX_BLOCKS;
    if (vec) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(adc_list_sample_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        hipLaunchKernelGGL(adc_list_sample_kernel<true>, dim3(blocks), dim3(ADC_LIST_THREADS), shmem, s, table, M, codes, rowmap,
                           n_vis, count, out);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(adc_list_sample_kernel<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        hipLaunchKernelGGL(adc_list_sample_kernel<false>, dim3(blocks), dim3(ADC_LIST_THREADS), shmem, s, table, M, codes, rowmap,
                           n_vis, count, out);
    }
}

// ---- exact scan ------------------------------------------------------------------------------------------------------
struct AdcListArgs {
    const float *table; // [M*256] of this query
    int M;
    const uint8_t *codes;
    const uint32_t *rowmap;
    int64_t pos_begin, pos_end;
    int slot;
    CandState cs;
    int boot;
};

// adc_scan_kernel's boot and admission modes over positions [pos_begin, pos_end)
template <bool VEC16>
__global__ __launch_bounds__(ADC_LIST_THREADS) void adc_list_scan_kernel(AdcListArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float tab[];
    const int M = a.M;
    for (int i = threadIdx.x; i < M * 256; i += ADC_LIST_THREADS) tab[i] = a.table[i];
    __syncthreads();
    const uint64_t tau = a.cs.tau[a.slot];
    uint64_t *list = a.cs.lists + (size_t)a.slot * a.cs.cap;
    for (int64_t pos = a.pos_begin + (int64_t)blockIdx.x * ADC_LIST_THREADS + threadIdx.x; pos < a.pos_end;
         pos += (int64_t)gridDim.x * ADC_LIST_THREADS) {
        const uint32_t row = a.rowmap[pos];
        const float sum = adc_row_sum<VEC16>(tab, a.codes + (int64_t)row * M, M);
        const uint64_t ent = pack_entry(adc_distance(sum), row);
        if (a.boot) {
            list[pos - a.pos_begin] = ent; // (the host keeps a boot chunk within the list: chunk_end_host)
        } else if (ent < tau) {
            const uint32_t at = atomicAdd(&a.cs.cnt[a.slot], 1u);
            if (at < a.cs.cap) list[at] = ent;
        }
    }
}

void launch_adc_list_scan(const float *table, int M, const uint8_t *codes, const uint32_t *rowmap, int64_t pos_begin,
                          int64_t pos_end, int slot, CandState cs, bool boot, hipStream_t s)
{
    if (pos_end <= pos_begin) return;
    AdcListArgs a{table, M, codes, rowmap, pos_begin, pos_end, slot, cs, boot ? 1 : 0};
    const size_t shmem = (size_t)M * 256 * sizeof(float);
    int64_t blocks = (pos_end - pos_begin + ADC_LIST_THREADS - 1) / ADC_LIST_THREADS;
    if (blocks > ADC_LIST_MAX_BLOCKS) blocks = ADC_LIST_MAX_BLOCKS;
    const bool vec = (M % 16 == 0) && ((reinterpret_cast<uintptr_t>(codes) & 15) == 0);
    if (vec) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(adc_list_scan_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        hipLaunchKernelGGL(adc_list_scan_kernel<true>, dim3((unsigned)blocks), dim3(ADC_LIST_THREADS), shmem, s, a);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(adc_list_scan_kernel<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        hipLaunchKernelGGL(adc_list_scan_kernel<false>, dim3((unsigned)blocks), dim3(ADC_LIST_THREADS), shmem, s, a);
    }
}

// ---- byte-table prefilter --------------------------------------------------------------------------------------------
struct AdcListPreArgs {
    const uint8_t *qtab; // [M*256] byte table of this query
    const int *params;   // {s_tau, ok}
    const uint8_t *codes;
    const uint32_t *rowmap;
    int64_t n_vis;
    uint32_t *cand;      // candidate ROWS
    uint32_t cand_cap;
    uint32_t *cand_cnt;  // [0] = count (may exceed cand_cap -> overflow, seen by adc_exact_candidates_kernel)
    // second query of a two-query pass (NQ == 2): the rows are gathered ONCE for both
    const uint8_t *qtab2;
    const int *params2;
    uint32_t *cand2;
    uint32_t *cand_cnt2;
};

// {s_tau of each query or -1 where its prefilter is unusable}; false = neither query has anything to do here (uniform)
template <int NQ> __device__ __forceinline__ bool list_pre_bounds(const AdcListPreArgs &a, int &s_tau, int &s_tau2)
{
    const int ok1 = a.params[1], ok2 = NQ == 2 ? a.params2[1] : 0;
    s_tau = ok1 ? a.params[0] : -1;
    s_tau2 = (NQ == 2 && ok2) ? a.params2[0] : -1;
    return ok1 != 0 || ok2 != 0;
}

template <int NQ> __device__ __forceinline__ void list_pre_admit(const AdcListPreArgs &a, uint32_t row, uint32_t S, uint32_t S2,
                                                                  int s_tau, int s_tau2)
{
    if ((int)S <= s_tau) {
        const uint32_t at = atomicAdd(a.cand_cnt, 1u);
        if (at < a.cand_cap) a.cand[at] = row;
    }
    if (NQ == 2 && (int)S2 <= s_tau2) {
        const uint32_t at = atomicAdd(a.cand_cnt2, 1u);
        if (at < a.cand_cap) a.cand2[at] = row;
    }
}

// adc_prefilter_kernel's arithmetic, a lane per list position.  The byte tables sit in LDS, the second M * 256 bytes behind
// the first.  Registers hold the current position's row (MCH x 16 B) and, loaded before the gathers of the current one start,
// the next position's; the row id of the position after that is in flight as well, so a lane's dependent loads (id, then
// codes) are each one step ahead of their use.  The two-query form at M = 96 has no registers left for the row ahead (1024
// threads leave 128 VGPRs a lane, and its 192 gathers in flight take most of them): it fetches the current row only.
template <int MCH, int NQ>
__global__ __launch_bounds__(ADC_LIST_THREADS) void adc_list_prefilter_kernel(AdcListPreArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_u8[];
    constexpr int M = MCH * 16;
    unsigned char *tab = smem_u8;
    const int tid = threadIdx.x;
    int s_tau, s_tau2;
    if (!list_pre_bounds<NQ>(a, s_tau, s_tau2)) return;
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.qtab);
        uint4 *dst = reinterpret_cast<uint4 *>(tab);
        for (int i = tid; i < M * 16; i += ADC_LIST_THREADS) dst[i] = src[i];
        if (NQ == 2) {
            const uint4 *src2 = reinterpret_cast<const uint4 *>(a.qtab2);
            for (int i = tid; i < M * 16; i += ADC_LIST_THREADS) dst[M * 16 + i] = src2[i];
        }
    }
    __syncthreads();
    constexpr bool AHEAD = !(NQ == 2 && MCH >= 6);
    const int64_t stride = (int64_t)gridDim.x * ADC_LIST_THREADS;
    int64_t pos = (int64_t)blockIdx.x * ADC_LIST_THREADS + tid;
    if (pos >= a.n_vis) return; // (no barrier follows)
    auto fetch = [&](uint32_t row, uint4 (&c)[MCH]) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 *src = reinterpret_cast<const u32x4 *>(a.codes + (int64_t)row * M);
#pragma unroll
        for (int i = 0; i < MCH; i++) {
            const u32x4 w = __builtin_nontemporal_load(src + i); // the visible rows pass through once
            c[i] = make_uint4(w.x, w.y, w.z, w.w);
        }
    };
    uint32_t row = a.rowmap[pos];
    uint32_t row_next = pos + stride < a.n_vis ? a.rowmap[pos + stride] : 0u;
    uint4 c[MCH], cn[MCH];
    fetch(row, c);
    for (; pos < a.n_vis; pos += stride) {
        const bool more = pos + stride < a.n_vis;
        uint32_t row_after = 0u;
        if (more) {
            if (AHEAD) fetch(row_next, cn);
            if (pos + 2 * stride < a.n_vis) row_after = a.rowmap[pos + 2 * stride];
        }
        uint32_t S = 0, S2 = 0;
#pragma unroll
        for (int g = 0; g < MCH; g++) {
            const uint32_t w[4] = {c[g].x, c[g].y, c[g].z, c[g].w};
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int j = g * 16 + t * 4 + b;
                    const uint32_t code = (w[t] >> (8 * b)) & 0xffu;
                    S += tab[j * 256 + code];
                    if (NQ == 2) S2 += tab[M * 256 + j * 256 + code];
                }
        }
        list_pre_admit<NQ>(a, row, S, S2, s_tau, s_tau2);
        if (more) {
            if (AHEAD) {
#pragma unroll
                for (int i = 0; i < MCH; i++) c[i] = cn[i];
            } else {
                fetch(row_next, c);
            }
        }
        row = row_next;
        row_next = row_after;
    }
}

// any M (or misaligned codes or tables): single bytes straight from global memory, one query per pass
__global__ __launch_bounds__(ADC_LIST_THREADS) void adc_list_prefilter_generic_kernel(AdcListPreArgs a, int M)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_u8[];
    int s_tau, s_tau2;
    if (!list_pre_bounds<1>(a, s_tau, s_tau2)) return;
    for (int i = threadIdx.x; i < M * 256; i += ADC_LIST_THREADS) smem_u8[i] = a.qtab[i];
    __syncthreads();
    for (int64_t pos = (int64_t)blockIdx.x * ADC_LIST_THREADS + threadIdx.x; pos < a.n_vis;
         pos += (int64_t)gridDim.x * ADC_LIST_THREADS) {
        const uint32_t row = a.rowmap[pos];
        const uint8_t *c = a.codes + (int64_t)row * M;
        uint32_t S = 0;
        for (int j = 0; j < M; j++) S += smem_u8[j * 256 + c[j]];
        list_pre_admit<1>(a, row, S, 0u, s_tau, s_tau2);
    }
}

static unsigned list_blocks(int64_t n_vis)
{
    const int64_t blocks = (n_vis + ADC_LIST_THREADS - 1) / ADC_LIST_THREADS;
    return (unsigned)(blocks > ADC_LIST_MAX_BLOCKS ? ADC_LIST_MAX_BLOCKS : blocks);
}

template <int MCH, int NQ> static bool try_list_prefilter(const AdcListPreArgs &a, hipStream_t s)
{
    const size_t shmem = (size_t)NQ * (MCH * 16) * 256;
    if (shmem > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(adc_list_prefilter_kernel<MCH, NQ>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    hipLaunchKernelGGL((adc_list_prefilter_kernel<MCH, NQ>), dim3(list_blocks(a.n_vis)), dim3(ADC_LIST_THREADS), shmem, s, a);
    return true;
}

// (M = 128 has a single form only, as in launch_adc_prefilter2: two tables' gathers in flight do not fit the registers)
template <int NQ> static bool list_prefilter_aligned(const AdcListPreArgs &a, int M, hipStream_t s)
{
    if (NQ == 2 && M / 16 == 8) return false;
    switch (M / 16) {
    case 1: return try_list_prefilter<1, NQ>(a, s);
    case 2: return try_list_prefilter<2, NQ>(a, s);
    case 3: return try_list_prefilter<3, NQ>(a, s);
    case 4: return try_list_prefilter<4, NQ>(a, s);
    case 6: return try_list_prefilter<6, NQ>(a, s);
    case 8: return try_list_prefilter<8, 1>(a, s);
    default: return false;
    }
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// two queries per pass over the list; false = no two-query form for this M or these addresses (the caller runs two single passes)
bool launch_adc_list_prefilter2(const uint8_t *qtab, const int *params, uint32_t *cand, uint32_t *cand_cnt, const uint8_t *qtab2,
                                const int *params2, uint32_t *cand2, uint32_t *cand_cnt2, int M, const uint8_t *codes,
                                const uint32_t *rowmap, int64_t n_vis, uint32_t cand_cap, hipStream_t s)
{
    if (M % 16 != 0 || !aligned16(codes) || !aligned16(qtab) || !aligned16(qtab2)) return false;
    if (n_vis <= 0) return true;
    const AdcListPreArgs a{qtab, params, codes, rowmap, n_vis, cand, cand_cap, cand_cnt, qtab2, params2, cand2, cand_cnt2};
    return list_prefilter_aligned<2>(a, M, s);
}

bool launch_adc_list_prefilter(const uint8_t *qtab, const int *params, int M, const uint8_t *codes, const uint32_t *rowmap,
                               int64_t n_vis, uint32_t *cand, uint32_t cand_cap, uint32_t *cand_cnt, hipStream_t s)
{
    if (n_vis <= 0) return true;
    const AdcListPreArgs a{qtab, params, codes, rowmap, n_vis, cand, cand_cap, cand_cnt, nullptr, nullptr, nullptr, nullptr};
    if (M % 16 == 0 && aligned16(codes) && aligned16(qtab) && list_prefilter_aligned<1>(a, M, s)) return true;
    const size_t shmem = (size_t)M * 256;
    if (shmem > 160 * 1024) return false;
    if (shmem > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(adc_list_prefilter_generic_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    hipLaunchKernelGGL(adc_list_prefilter_generic_kernel, dim3(list_blocks(a.n_vis)), dim3(ADC_LIST_THREADS), shmem, s, a, M);
    return true;
}

} // namespace lb
