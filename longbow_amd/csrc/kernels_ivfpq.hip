// kernels_ivfpq.hip -- the IVF-PQ index (ivfpq.hip; semantics in include/longbow_gpu.h, lb_gpu_ivfpq_*): the list-major copy of
// the codes and the exact ADC scan of a query's probed lists, or under a row filter of their visible entries.  The plan, the
// selection, the counting sort and the build of the visible lists are the IVF-Flat index's (kernels_ivf.hip), the table and the
// codec the PQ handle's (kernels_pq.hip, kernels_pq2.hip).
//
// The arithmetic is adc_scan_kernel's, through the same device functions (lb_exact.h): the f32 sum of table[j * 256 + code[j]]
// in j order, float(sqrt(double(sum))), pack_entry(distance, row).  Nothing is admitted against a threshold: every scanned
// position leaves one key and ivf_select_kernel takes the k smallest.
#include "lb_device.h"
#include "lb_exact.h"
#include "lb_ivfpq.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

// ---- the list-major copy -----------------------------------------------------------------------------------------------------
// A wave takes 64 consecutive positions: their 64 row ids are one 256-byte load, each row is gathered as M / 16 16-byte pieces
// (single bytes when M % 16 != 0) and the run leaves as one contiguous block of 64 * M bytes, piece p of the run from lane
// p % 64.  No load leaves [codes, codes + n * M) and no store [lcodes, lcodes + n * M).
constexpr int IPQ_PERM_THREADS = 256;

template <bool VEC16>
__global__ __launch_bounds__(IPQ_PERM_THREADS) void ivfpq_permute_kernel(const uint8_t *codes, const uint32_t *rows, int64_t n, int M,
                                                                         uint8_t *lcodes)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = VEC16 ? M / 16 : M;  // pieces a row
    const int width = VEC16 ? 16 : 1;    // bytes a piece
    for (int64_t p0 = ((int64_t)blockIdx.x * (IPQ_PERM_THREADS / 64) + wave) * 64; p0 < n; p0 += (int64_t)gridDim.x * IPQ_PERM_THREADS) {
        const int cnt = (int)std::min<int64_t>(64, n - p0);
        const uint32_t rid = lane < cnt ? rows[p0 + lane] : 0u;
        uint8_t *dst = lcodes + p0 * M;
        for (int i = 0; i < per; i++) { // (every lane walks all of it: the shuffle reads lanes that hold no piece)
            const int p = i * 64 + lane;
            const int r = p / per, piece = p - r * per;
            const uint32_t row = __shfl(rid, r);
            if (r >= cnt || (int64_t)row >= n) continue;
            const uint8_t *src = codes + (int64_t)row * M + piece * width;
            if (VEC16) *reinterpret_cast<uint4 *>(dst + (int64_t)p * 16) = *reinterpret_cast<const uint4 *>(src);
            else dst[p] = *src;
        }
    }
}

void launch_ivfpq_permute(const uint8_t *codes, const uint32_t *rows, int64_t n, int M, uint8_t *lcodes, hipStream_t s)
{
    if (n <= 0) return;
    const bool vec = M % 16 == 0 && ((reinterpret_cast<uintptr_t>(codes) | reinterpret_cast<uintptr_t>(lcodes)) & 15) == 0;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + IPQ_PERM_THREADS - 1) / IPQ_PERM_THREADS, 8192);
    if (vec) hipLaunchKernelGGL(ivfpq_permute_kernel<true>, dim3(blocks), dim3(IPQ_PERM_THREADS), 0, s, codes, rows, n, M, lcodes);
    else hipLaunchKernelGGL(ivfpq_permute_kernel<false>, dim3(blocks), dim3(IPQ_PERM_THREADS), 0, s, codes, rows, n, M, lcodes);
}

// ---- the scan ----------------------------------------------------------------------------------------------------------------
// Grid: y = the query of the batch, x = G workgroups that stride over the query's positions t in [0, P_q) in tiles of IPQ_TILE.
// The tiles are flat over the concatenation of the probed lists, so a short list costs nothing and the work is even.
// A workgroup copies its query's table to LDS once (M * 1024 bytes, in 16-byte pieces) and, where they fit beside it (SEG_LDS),
// the query's seg[np + 1] and the probed lists' first positions; otherwise those two stay in global memory (a table of 159
// subspaces leaves 1 KB of the 160 KB, and a search of every list may have 65,536 probes).  One barrier.  Then a lane owns
// position t: slot s = the last one with seg[s] <= t, pos = off[probe[s]] + (t - seg[s]), the code row lcodes[pos], the row
// number rows[pos].  Plain loads: other queries of the batch probe the same lists.  No atomics, no waits on other workgroups.
// MCH: M / 16 at compile time (the row's 16-byte loads are issued together); 0: M % 16 == 0 at run time; -1: single bytes.
// VIS: the search runs under a row filter.  a.L is then the visible lists, whose entries are positions into the lists of all
// rows: the t-th visible entry is vp = voff[probe[s]] + (t - seg[s]), one coalesced 4-byte load gives pos = vlist[vp], and from
// there on the lane does what it does without a filter, at a position that stays inside the probed list's run of lcodes; the
// row number comes from `rows`, the rows of all lists (unused without VIS, where a.L.rows is that array).  vp and pos are
// checked against nvis and n before they index anything.
template <int MCH, bool SEG_LDS, bool VIS>
__global__ __launch_bounds__(IPQ_TILE) void ivfpq_scan_kernel(IvfBatch a, const float *tables, int M_rt, const uint8_t *lcodes, int64_t n,
                                                              const uint32_t *rows, int64_t nvis)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int M = MCH > 0 ? MCH * 16 : M_rt;
    const int q = blockIdx.y, tid = threadIdx.x, np = a.np;
    const uint32_t *gseg = a.seg + (int64_t)q * (np + 1);
    const int64_t *gprobe = a.probes + (int64_t)q * np;
    const uint32_t P = gseg[np];
    if ((uint64_t)blockIdx.x * IPQ_TILE >= P) return; // (the whole workgroup: nothing waits at the barrier below)
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(tables + (int64_t)q * M * 256);
        f32x4 *dst = reinterpret_cast<f32x4 *>(smem);
        for (int i = tid; i < M * 64; i += IPQ_TILE) dst[i] = src[i];
    }
    uint32_t *lseg = reinterpret_cast<uint32_t *>(smem + M * 256); // [np + 1], then the lists' first positions [np]
    uint32_t *lbase = lseg + np + 1;
    if (SEG_LDS) {
        for (int i = tid; i <= np; i += IPQ_TILE) {
            lseg[i] = gseg[i];
            if (i < np) {
                const int64_t l = gprobe[i];
                lbase[i] = l >= 0 && l < a.L.nlist ? a.L.off[l] : 0xffffffffu; // (such a slot holds no position: the plan gave it none)
            }
        }
    }
    __syncthreads();
    const uint32_t *seg = SEG_LDS ? lseg : gseg;
    uint64_t *keys = a.keys + (int64_t)q * a.pmax;
    for (uint32_t t = blockIdx.x * IPQ_TILE + tid; t < P; t += gridDim.x * IPQ_TILE) { // (P <= pmax < 2^31)
        int lo = 0, hi = np; // seg[lo] <= t < seg[hi] throughout: seg[0] = 0, seg[np] = P
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (seg[mid] <= t) lo = mid;
            else hi = mid;
        }
        uint32_t base;
        if (SEG_LDS) {
            base = lbase[lo];
        } else {
            const int64_t l = gprobe[lo];
            base = l >= 0 && l < a.L.nlist ? a.L.off[l] : 0xffffffffu;
        }
        uint64_t pos = (uint64_t)base + (t - seg[lo]);
        if (VIS) pos = pos < (uint64_t)nvis ? a.L.rows[pos] : ~0ull; // (the visible entry -> its position)
        uint64_t key = kEntryMax;
        if (pos < (uint64_t)n) { // always: a non-empty slot is a list of the handle
            const uint8_t *c = lcodes + pos * (uint64_t)M;
            float sum = 0.f;
            if (MCH > 0) {
                uint4 v[MCH > 0 ? MCH : 1];
#pragma unroll
                for (int g = 0; g < MCH; g++) v[g] = *reinterpret_cast<const uint4 *>(c + g * 16);
#pragma unroll
                for (int g = 0; g < MCH; g++) sum = adc_add16(sum, smem, g, v[g]);
            } else if (MCH == 0) {
                sum = adc_row_sum<true>(smem, c, M);
            } else {
                sum = adc_row_sum<false>(smem, c, M);
            }
            key = pack_entry(adc_distance(sum), VIS ? rows[pos] : a.L.rows[pos]);
        }
        keys[t] = key;
    }
}

template <int MCH, bool VIS>
static void launch_ivfpq_scan_m(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, const uint32_t *rows,
                                int64_t nvis, hipStream_t s)
{
    const size_t table = (size_t)M * 256 * sizeof(float), segs = ((size_t)2 * a.np + 1) * sizeof(uint32_t);
    const bool seg_lds = table + segs <= (size_t)160 * 1024;
    const size_t shmem = table + (seg_lds ? segs : 0);
    const dim3 grid((unsigned)ivfpq_scan_groups(a.nq, a.pmax), (unsigned)a.nq);
    if (seg_lds) {
        if (shmem > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ivfpq_scan_kernel<MCH, true, VIS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)shmem);
        hipLaunchKernelGGL((ivfpq_scan_kernel<MCH, true, VIS>), grid, dim3(IPQ_TILE), shmem, s, a, tables, M, lcodes, n, rows, nvis);
    } else {
        if (shmem > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ivfpq_scan_kernel<MCH, false, VIS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)shmem);
        hipLaunchKernelGGL((ivfpq_scan_kernel<MCH, false, VIS>), grid, dim3(IPQ_TILE), shmem, s, a, tables, M, lcodes, n, rows, nvis);
    }
}

template <bool VIS>
static void launch_ivfpq_scan_v(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, const uint32_t *rows, int64_t nvis,
                                hipStream_t s)
{
    if (a.nq <= 0 || n <= 0) return;
    const bool vec = M % 16 == 0 && (reinterpret_cast<uintptr_t>(lcodes) & 15) == 0; // (tables: 16-byte aligned in every form)
    if (!vec) return launch_ivfpq_scan_m<-1, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    switch (M / 16) { // the forms adc_scan_dma_kernel has
    case 1: return launch_ivfpq_scan_m<1, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 2: return launch_ivfpq_scan_m<2, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 3: return launch_ivfpq_scan_m<3, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 4: return launch_ivfpq_scan_m<4, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 6: return launch_ivfpq_scan_m<6, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 8: return launch_ivfpq_scan_m<8, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    default: return launch_ivfpq_scan_m<0, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    }
}

void launch_ivfpq_scan(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, hipStream_t s)
{
    launch_ivfpq_scan_v<false>(a, tables, M, lcodes, n, nullptr, 0, s);
}

void launch_ivfpq_scan_visible(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, const uint32_t *rows, int64_t nvis,
                               hipStream_t s)
{
    if (nvis <= 0) return; // (every seg is 0: no key is read)
    launch_ivfpq_scan_v<true>(a, tables, M, lcodes, n, rows, nvis, s);
}

} // namespace lb
