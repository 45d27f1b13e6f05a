// kernels_ivfpq.hip -- the IVF-PQ index (ivfpq.hip; semantics in include/longbow_gpu.h, lb_gpu_ivfpq_*): the list-major copy of
// the codes and the exact ADC scan of a query's probed lists, or under a row filter of their visible entries.  The plan, the
// selection, the counting sort and the build of the visible lists are the IVF-Flat index's (kernels_ivf.hip), the table and the
// codec the PQ handle's (kernels_pq.hip, kernels_pq2.hip).  For a residual handle also: the residuals of rows and of (query, probed
// list) pairs, and the scan under a table per pair (ivfpq_rscan_kernel), strided or from a work list.
//
// The arithmetic is adc_scan_kernel's, through the same device functions (lb_exact.h): the f32 sum of table[j * 256 + code[j]]
// in j order, float(sqrt(double(sum))), pack_entry(distance, row).  Nothing is admitted against a threshold: every scanned
// position leaves one key and ivf_select_kernel takes the k smallest.
#include "lb_device.h"
#include "lb_exact.h"
#include "lb_ivfpq.h"
#include "lb_select.h"

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

// ---- residual codes ----------------------------------------------------------------------------------------------------------
// res(v, l)[i] = v[i] - C[l][i]: one f32 subtraction a component, stored as it is (the contraction pragma above holds here too,
// and nothing follows the subtraction).  A thread an element; reads of C stay inside [0, nlist) rows.
constexpr int IPQ_RES_THREADS = 256;

__global__ __launch_bounds__(IPQ_RES_THREADS) void ivfpq_residual_rows_kernel(const float *X, const uint32_t *assign, const float *C, int64_t cnt,
                                                                              int dims, int nlist, float *out)
{
    const int64_t total = cnt * dims;
    for (int64_t e = (int64_t)blockIdx.x * IPQ_RES_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * IPQ_RES_THREADS) {
        const int64_t r = e / dims;
        const int i = (int)(e - r * dims);
        const uint32_t l = assign[r];
        if (l >= (uint32_t)nlist) continue; // (no list of the handle: nothing is written)
        out[e] = X[e] - C[(int64_t)l * dims + i];
    }
}

void launch_ivfpq_residual_rows(const float *X, const uint32_t *assign, const float *C, int64_t cnt, int dims, int nlist, float *out, hipStream_t s)
{
    if (cnt <= 0 || dims <= 0) return;
    const unsigned blocks = (unsigned)std::min<int64_t>((cnt * dims + IPQ_RES_THREADS - 1) / IPQ_RES_THREADS, 8192);
    hipLaunchKernelGGL(ivfpq_residual_rows_kernel, dim3(blocks), dim3(IPQ_RES_THREADS), 0, s, X, assign, C, cnt, dims, nlist, out);
}

// pair = q * ns + (slot - s0) over the batch's queries and the slots [s0, s0 + ns) of each
__global__ __launch_bounds__(IPQ_RES_THREADS) void ivfpq_residual_queries_kernel(IvfBatch a, int s0, int ns, const float *C, float *rq)
{
    const int dims = a.D;
    const int64_t total = (int64_t)a.nq * ns * dims;
    for (int64_t e = (int64_t)blockIdx.x * IPQ_RES_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * IPQ_RES_THREADS) {
        const int64_t pair = e / dims;
        const int i = (int)(e - pair * dims);
        const int64_t q = pair / ns;
        const int slot = s0 + (int)(pair - q * ns);
        const int64_t l = a.probes[q * a.np + slot];
        rq[e] = l >= 0 && l < a.L.nlist ? a.Q[q * dims + i] - C[l * dims + i] : 0.f; // (no list: zeros, and the plan gave it no positions)
    }
}

void launch_ivfpq_residual_queries(const IvfBatch &a, int s0, int ns, const float *C, float *rq, hipStream_t s)
{
    if (a.nq <= 0 || ns <= 0 || a.D <= 0) return;
    const int64_t total = (int64_t)a.nq * ns * a.D;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + IPQ_RES_THREADS - 1) / IPQ_RES_THREADS, 8192);
    hipLaunchKernelGGL(ivfpq_residual_queries_kernel, dim3(blocks), dim3(IPQ_RES_THREADS), 0, s, a, s0, ns, C, rq);
}

// ---- the residual scan -------------------------------------------------------------------------------------------------------
// A query has a table per probed list, so the work unit is a pair, not a query.  Grid: x = the pair (q, slot) of the launch (a
// batch of 1024 queries at 65,536 probes is beyond what y takes), y = G workgroups that stride over THAT slot's positions
// i in [0, seg[slot + 1] - seg[slot]) in tiles of IPQ_TILE.  A workgroup whose first tile starts past the slot's length returns
// before it touches LDS: an empty list, or a slot that is no list, costs a launch slot and nothing else.  The others copy their
// pair's table to LDS once (M * 1024 bytes, in 16-byte pieces); they read the slot's two seg values, the query's total (the bound
// of its keys) and one list base, so nothing else is kept in LDS.  One barrier.  Then a lane does what ivfpq_scan_kernel's does: pos = off[probe] + i, under VIS
// vp = voff[probe] + i and pos = vlist[vp] (vp < nvis and pos < n checked before either indexes anything), the code row
// lcodes[pos] by the same MCH forms, the same arithmetic, and keys[q][seg[slot] + i] at the t the plan assigned, so the
// selection and the stats are the plain handle's.  Plain loads and stores, no atomics, no waits on other workgroups.
// The body is this kernel's own: ivfpq_scan_kernel keeps its text and with it its registers.
//
// With few workgroups a pair (many pairs) the longest list is a serial tail of hundreds of tiles in one workgroup.  The launcher
// then runs the scan from a work list (ivfpq_rscan_plan): grid x = the items, an item being a pair and a run of `run` consecutive
// tiles of its list.  item_off[pairs + 1] is the exclusive prefix sum of the pairs' item counts, ceil(ceil(len / IPQ_TILE) / run),
// written by ivfpq_rscan_items_kernel in one workgroup before the scan.  Workgroup w returns when w >= item_off[pairs]; else its
// pair is the last p with item_off[p] <= w (so that pair has items), by bisection over loads that are uniform over the workgroup,
// and its tiles are [(w - item_off[p]) * run, + run).  Everything after that is the strided form's, tile by tile.
__global__ __launch_bounds__(IPQ_TILE) void ivfpq_rscan_items_kernel(IvfBatch a, int s0, int ns, int run, uint32_t *item_off)
{
    __shared__ uint32_t wsum[IPQ_TILE / 64];
    const int64_t pairs = (int64_t)a.nq * ns;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0; // items of the pairs before this round's (the host's bound of them all is below 2^31)
    for (int64_t p0 = 0; p0 < pairs; p0 += IPQ_TILE) {
        const int64_t p = p0 + tid;
        uint32_t items = 0;
        if (p < pairs) {
            const int64_t q = p / ns;
            const int slot = s0 + (int)(p - q * ns);
            const uint32_t *gseg = a.seg + q * (a.np + 1);
            const uint32_t t0 = gseg[slot], t1 = std::min(gseg[slot + 1], gseg[a.np]);
            const uint32_t tiles = t1 > t0 ? (t1 - t0 + IPQ_TILE - 1) / IPQ_TILE : 0u;
            items = (tiles + run - 1) / run;
        }
        const uint32_t incl = wave_incl_scan(items, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < IPQ_TILE / 64; w++) {
            before += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        if (p < pairs) item_off[p] = carry + before + incl - items;
        carry += total;
        __syncthreads(); // (wsum is rewritten by the next round)
    }
    if (tid == 0) item_off[pairs] = carry;
}

template <int MCH, bool VIS>
__global__ __launch_bounds__(IPQ_TILE) void ivfpq_rscan_kernel(IvfBatch a, int s0, int ns, const float *tables, int M_rt, const uint8_t *lcodes,
                                                               int64_t n, const uint32_t *rows, int64_t nvis, const uint32_t *item_off, int run)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int M = MCH > 0 ? MCH * 16 : M_rt;
    int64_t pair = blockIdx.x;
    uint32_t tile = blockIdx.y, tile_end = 0xffffffffu, tile_step = gridDim.y; // the strided form
    if (item_off) {
        const int64_t pairs = (int64_t)a.nq * ns;
        const uint32_t w = blockIdx.x;
        if (w >= item_off[pairs]) return;
        int64_t lo = 0, hi = pairs; // item_off[lo] <= w < item_off[hi] throughout: item_off[0] = 0
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (item_off[mid] <= w) lo = mid;
            else hi = mid;
        }
        pair = lo;
        tile = (w - item_off[lo]) * (uint32_t)run;
        tile_end = tile + (uint32_t)run;
        tile_step = 1;
    }
    const int64_t q = pair / ns;
    const int slot = s0 + (int)(pair - q * ns), tid = threadIdx.x;
    const uint32_t *gseg = a.seg + q * (a.np + 1);
    const uint32_t P = gseg[a.np]; // (<= pmax: no key is written at or beyond it)
    const uint32_t t0 = gseg[slot], t1 = std::min(gseg[slot + 1], P); // (the plan's prefix sums: t0 <= t1 <= P always)
    const uint32_t len = t1 > t0 ? t1 - t0 : 0u;
    if ((uint64_t)tile * IPQ_TILE >= len) return; // (the whole workgroup: nothing waits at the barrier below)
    const int64_t l = a.probes[q * a.np + slot];
    const uint32_t base = l >= 0 && l < a.L.nlist ? a.L.off[l] : 0xffffffffu; // (a non-empty slot is a list of the handle)
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(tables + pair * M * 256);
        f32x4 *dst = reinterpret_cast<f32x4 *>(smem);
        for (int i = tid; i < M * 64; i += IPQ_TILE) dst[i] = src[i];
    }
    __syncthreads();
    uint64_t *keys = a.keys + q * a.pmax + t0;
    for (; tile < tile_end; tile += tile_step) { // (tile_step <= IPQ_GRID, and the first tile past len ends the loop: no wrap)
        const uint64_t i = (uint64_t)tile * IPQ_TILE + tid;
        if (i >= len) {
            if ((uint64_t)tile * IPQ_TILE >= len) break; // (the whole workgroup)
            continue;                                    // (a lane past the end of the last tile)
        }
        uint64_t pos = (uint64_t)base + i;
        if (VIS) pos = pos < (uint64_t)nvis ? a.L.rows[pos] : ~0ull; // (the visible entry -> its position)
        uint64_t key = kEntryMax;
        if (pos < (uint64_t)n) {
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
        keys[i] = key;
    }
}

template <int MCH, bool VIS>
static void launch_ivfpq_rscan_m(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n,
                                 const IvfpqRscanPlan &plan, const uint32_t *item_off, const uint32_t *rows, int64_t nvis, hipStream_t s)
{
    const size_t shmem = (size_t)M * 256 * sizeof(float);
    const int64_t pairs = (int64_t)a.nq * ns;
    const dim3 grid(plan.items ? (unsigned)plan.grid : (unsigned)pairs, plan.items ? 1u : (unsigned)plan.groups);
    if (shmem > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ivfpq_rscan_kernel<MCH, VIS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    hipLaunchKernelGGL((ivfpq_rscan_kernel<MCH, VIS>), grid, dim3(IPQ_TILE), shmem, s, a, s0, ns, tables, M, lcodes, n, rows, nvis,
                       plan.items ? item_off : nullptr, plan.run);
}

template <bool VIS>
static void launch_ivfpq_rscan_v(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n, int64_t maxlen,
                                 uint32_t *item_off, const uint32_t *rows, int64_t nvis, hipStream_t s)
{
    if (a.nq <= 0 || ns <= 0 || n <= 0 || s0 < 0 || s0 + ns > a.np) return;
    IvfpqRscanPlan plan = ivfpq_rscan_plan((int64_t)a.nq * ns, a.nq, a.pmax, maxlen);
    if (plan.items && !item_off) plan = IvfpqRscanPlan{false, ivfpq_rscan_groups((int64_t)a.nq * ns, maxlen), 0, 0};
    if (plan.items) hipLaunchKernelGGL(ivfpq_rscan_items_kernel, dim3(1), dim3(IPQ_TILE), 0, s, a, s0, ns, plan.run, item_off);
    const bool vec = M % 16 == 0 && (reinterpret_cast<uintptr_t>(lcodes) & 15) == 0; // (tables: 16-byte aligned in every form)
    if (!vec) return launch_ivfpq_rscan_m<-1, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    switch (M / 16) { // ivfpq_scan_kernel's forms
    case 1: return launch_ivfpq_rscan_m<1, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 2: return launch_ivfpq_rscan_m<2, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 3: return launch_ivfpq_rscan_m<3, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 4: return launch_ivfpq_rscan_m<4, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 6: return launch_ivfpq_rscan_m<6, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 8: return launch_ivfpq_rscan_m<8, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    default: return launch_ivfpq_rscan_m<0, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    }
}

void launch_ivfpq_rscan(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n, int64_t maxlen,
                        uint32_t *item_off, hipStream_t s)
{
    launch_ivfpq_rscan_v<false>(a, s0, ns, tables, M, lcodes, n, maxlen, item_off, nullptr, 0, s);
}

void launch_ivfpq_rscan_visible(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n, int64_t maxlen,
                                uint32_t *item_off, const uint32_t *rows, int64_t nvis, hipStream_t s)
{
    if (nvis <= 0) return; // (every seg is 0: no key is read)
    launch_ivfpq_rscan_v<true>(a, s0, ns, tables, M, lcodes, n, maxlen, item_off, rows, nvis, s);
}

} // namespace lb
