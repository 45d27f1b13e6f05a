// kernels_ivfpq4.hip -- the IVF-PQ4 index (ivfpq4.hip; semantics in include/longbow_gpu.h, lb_gpu_ivfpq4_*): the exact ADC scan of
// a query's probed lists over packed 4-bit codes (lb_pq4.h states the row layout), or under a row filter of their visible
// entries, with one table a query (ivfpq4_scan_kernel) or, for a residual handle, one a (query, probed list) pair
// (ivfpq4_rscan_kernel, strided or from a work list).  Everything else on the device is existing launchers: the plan, the
// selection and the visible lists are the IVF-Flat index's (kernels_ivf.hip), the list-major copy and the residuals the IVF-PQ
// index's (kernels_ivfpq.hip), the codec the PQ4 handle's (kernels_pq4.hip), the table kernels_pq.hip's at K = 16.
//
// The design around the table and the row.  A table is [M][16] f32, M * 64 bytes: 6 KB at M = 96 against the 96 KB of K = 256, so
// LDS no longer bounds a CU to one workgroup and the copy is a few loads a lane.  A subtable is 64 bytes, the 16 banks a lookup of
// one subspace touches: the lanes of a wave look subspace j up together, lanes with equal codes read one word (a broadcast) and
// different codes fall in different banks, so a lookup is one conflict-free ds_read_b32 at a compile-time offset j * 64 plus the
// nibble * 4.  A lane owns a position and holds its whole packed row in registers before the first lookup: P / 16 16-byte loads
// issued together (PCH of them at compile time for M = 32, 64, 96, 128, 192; a run-time loop for other P % 16 == 0), or single
// bytes for every other M, odd ones included, where the spare high nibble is never looked up.  The register lookup of
// kernels_pq4.hip (ds_bpermute_b32) is not used here: it needs every lane of a wave on, and a flat tile's lanes switch off at
// list ends.  No load leaves [lcodes, lcodes + n * P).
//
// The arithmetic is pq4_scan_kernel's: the f32 sum ((0 + t[0][c0]) + t[1][c1]) + ... in j order on one chain a lane, no
// reassociation (there is no product to contract; contraction is off all the same), float(sqrt(double(sum))),
// pack_entry(distance, row).  Nothing is admitted against a threshold: every scanned position leaves one key and
// ivf_select_kernel takes the k smallest.
#include "lb_device.h"
#include "lb_exact.h"
#include "lb_ivfpq4.h"
#include "lb_select.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

// ---- the row sum -------------------------------------------------------------------------------------------------------------
// the eight codes of a word (subspaces j0 .. j0 + 7, code b in bits [4b, 4b + 4)) onto the lane's chain; FULL: all eight exist,
// else each is asked against M (uniform over the wave)
template <bool FULL> __device__ __forceinline__ float ipq4_add_word(float sum, const float *lt, uint32_t w, int j0, int M)
{
#pragma unroll
    for (int b = 0; b < 8; b++)
        if (FULL || j0 + b < M) sum = sum + lt[(j0 + b) * PQ4_K + (int)((w >> (4 * b)) & 15u)];
    return sum;
}

template <bool FULL> __device__ __forceinline__ float ipq4_add16(float sum, const float *lt, const uint4 v, int j0, int M)
{
    sum = ipq4_add_word<FULL>(sum, lt, v.x, j0, M);
    sum = ipq4_add_word<FULL>(sum, lt, v.y, j0 + 8, M);
    sum = ipq4_add_word<FULL>(sum, lt, v.z, j0 + 16, M);
    return ipq4_add_word<FULL>(sum, lt, v.w, j0 + 24, M);
}

// The row of P bytes at c against the table lt in LDS.  PCH > 0: P = 16 PCH and M = 32 PCH, the loads issued before the first
// lookup; PCH == 0: P % 16 == 0 at run time (M = 2 P or 2 P - 1: the last piece asks against M); PCH < 0: single bytes.
template <int PCH> __device__ __forceinline__ float ipq4_row_sum(const float *lt, const uint8_t *c, int M, int P)
{
    float sum = 0.f;
    if constexpr (PCH > 0) {
        uint4 v[PCH];
#pragma unroll
        for (int g = 0; g < PCH; g++) v[g] = *reinterpret_cast<const uint4 *>(c + g * 16);
#pragma unroll
        for (int g = 0; g < PCH; g++) sum = ipq4_add16<true>(sum, lt, v[g], g * 32, M);
    } else if constexpr (PCH == 0) {
        for (int g = 0; g * 16 < P; g++) {
            const uint4 v = *reinterpret_cast<const uint4 *>(c + g * 16);
            sum = g * 32 + 32 <= M ? ipq4_add16<true>(sum, lt, v, g * 32, M) : ipq4_add16<false>(sum, lt, v, g * 32, M);
        }
    } else {
        for (int b = 0; b < P; b++) {
            const uint32_t byte = c[b];
            sum = sum + lt[(2 * b) * PQ4_K + (int)(byte & 15u)];
            if (2 * b + 1 < M) sum = sum + lt[(2 * b + 1) * PQ4_K + (int)(byte >> 4)]; // (the spare nibble of an odd M adds nothing)
        }
    }
    return sum;
}

// what a lane leaves for the position `pos` of the walked lists: under VIS `pos` is a visible entry, whose position in the lists
// of all rows is a.L.rows[pos]; vp < nvis and pos < n are checked before either indexes anything
template <int PCH, bool VIS>
__device__ __forceinline__ uint64_t ipq4_key(const IvfBatch &a, const float *lt, const uint8_t *lcodes, uint64_t pos, int M, int P, int64_t n,
                                             const uint32_t *rows, int64_t nvis)
{
    if (VIS) pos = pos < (uint64_t)nvis ? a.L.rows[pos] : ~0ull;
    if (pos >= (uint64_t)n) return kEntryMax; // never: a non-empty slot is a list of the handle
    const float sum = ipq4_row_sum<PCH>(lt, lcodes + pos * (uint64_t)P, M, P);
    return pack_entry(adc_distance(sum), VIS ? rows[pos] : a.L.rows[pos]);
}

// the table of M * 16 floats at src -> LDS, in 16-byte pieces
__device__ __forceinline__ void ipq4_table_to_lds(float *lt, const float *src, int M, int tid)
{
    const f32x4 *s4 = reinterpret_cast<const f32x4 *>(src);
    f32x4 *d4 = reinterpret_cast<f32x4 *>(lt);
    for (int i = tid; i < M * (PQ4_K / 4); i += IPQ_TILE) d4[i] = s4[i];
}

// ---- the plain scan ----------------------------------------------------------------------------------------------------------
// Grid and tiling are ivfpq_scan_kernel's: y = the query of the batch, x = G workgroups (ivfpq_scan_groups) that stride over the
// query's positions t in [0, P_q) in tiles of IPQ_TILE, flat over the concatenation of the probed lists.  A workgroup copies its
// query's table to LDS once and, where they fit beside it (SEG_LDS), the query's seg[np + 1] and the probed lists' first
// positions.  One barrier.  Then a lane owns position t: slot s = the last one with seg[s] <= t, pos = off[probe[s]] + (t -
// seg[s]), the packed row lcodes[pos], keys[q][t].  Plain loads and stores, no atomics, no waits on other workgroups.
template <int PCH, bool SEG_LDS, bool VIS>
__global__ __launch_bounds__(IPQ_TILE) void ivfpq4_scan_kernel(IvfBatch a, const float *tables, int M_rt, const uint8_t *lcodes, int64_t n,
                                                               const uint32_t *rows, int64_t nvis)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int M = PCH > 0 ? PCH * 32 : M_rt, P = PCH > 0 ? PCH * 16 : (M_rt + 1) / 2;
    const int q = blockIdx.y, tid = threadIdx.x, np = a.np;
    const uint32_t *gseg = a.seg + (int64_t)q * (np + 1);
    const int64_t *gprobe = a.probes + (int64_t)q * np;
    const uint32_t Pq = gseg[np];
    if ((uint64_t)blockIdx.x * IPQ_TILE >= Pq) return; // (the whole workgroup: nothing waits at the barrier below)
    ipq4_table_to_lds(smem, tables + (int64_t)q * M * PQ4_K, M, tid);
    uint32_t *lseg = reinterpret_cast<uint32_t *>(smem + M * PQ4_K); // [np + 1], then the lists' first positions [np]
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
    for (uint32_t t = blockIdx.x * IPQ_TILE + tid; t < Pq; t += gridDim.x * IPQ_TILE) { // (Pq <= pmax < 2^31)
        int lo = 0, hi = np; // seg[lo] <= t < seg[hi] throughout: seg[0] = 0, seg[np] = Pq
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
        keys[t] = ipq4_key<PCH, VIS>(a, smem, lcodes, (uint64_t)base + (t - seg[lo]), M, P, n, rows, nvis);
    }
}

template <int PCH, bool VIS>
static void launch_ivfpq4_scan_m(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, const uint32_t *rows,
                                 int64_t nvis, hipStream_t s)
{
    const size_t table = (size_t)M * PQ4_K * sizeof(float), segs = ((size_t)2 * a.np + 1) * sizeof(uint32_t);
    const bool seg_lds = table + segs <= (size_t)160 * 1024;
    const size_t shmem = table + (seg_lds ? segs : 0);
    const dim3 grid((unsigned)ivfpq_scan_groups(a.nq, a.pmax), (unsigned)a.nq);
    if (seg_lds) {
        if (shmem > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ivfpq4_scan_kernel<PCH, true, VIS>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        hipLaunchKernelGGL((ivfpq4_scan_kernel<PCH, true, VIS>), grid, dim3(IPQ_TILE), shmem, s, a, tables, M, lcodes, n, rows, nvis);
    } else {
        hipLaunchKernelGGL((ivfpq4_scan_kernel<PCH, false, VIS>), grid, dim3(IPQ_TILE), shmem, s, a, tables, M, lcodes, n, rows, nvis);
    }
}

// which row form serves M: PCH of ipq4_row_sum
static int ipq4_form(int M, const uint8_t *lcodes)
{
    const int P = pq4_row_bytes(M);
    if (P % 16 != 0 || (reinterpret_cast<uintptr_t>(lcodes) & 15) != 0) return -1; // (tables: 16-byte aligned in every form)
    const int pch = P / 16;
    return M == 32 * pch && (pch <= 4 || pch == 6) ? pch : 0;
}

template <bool VIS>
static void launch_ivfpq4_scan_v(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, const uint32_t *rows,
                                 int64_t nvis, hipStream_t s)
{
    if (a.nq <= 0 || n <= 0) return;
    switch (ipq4_form(M, lcodes)) {
    case 1: return launch_ivfpq4_scan_m<1, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 2: return launch_ivfpq4_scan_m<2, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 3: return launch_ivfpq4_scan_m<3, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 4: return launch_ivfpq4_scan_m<4, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 6: return launch_ivfpq4_scan_m<6, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    case 0: return launch_ivfpq4_scan_m<0, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    default: return launch_ivfpq4_scan_m<-1, VIS>(a, tables, M, lcodes, n, rows, nvis, s);
    }
}

void launch_ivfpq4_scan(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, hipStream_t s)
{
    launch_ivfpq4_scan_v<false>(a, tables, M, lcodes, n, nullptr, 0, s);
}

void launch_ivfpq4_scan_visible(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, const uint32_t *rows,
                                int64_t nvis, hipStream_t s)
{
    if (nvis <= 0) return; // (every seg is 0: no key is read)
    launch_ivfpq4_scan_v<true>(a, tables, M, lcodes, n, rows, nvis, s);
}

// ---- the residual scan -------------------------------------------------------------------------------------------------------
// A query has a table per probed list, so the work unit is a pair (q, slot), as in ivfpq_rscan_kernel.  Strided: grid x = the pair
// of the launch, y = G workgroups that stride over that slot's positions i in [0, seg[slot + 1] - seg[slot]) in tiles of
// IPQ_TILE.  From a work list (ivfpq_rscan_plan, where the longest list would be a serial tail): grid x = the items, an item being
// a pair and a run of `run` consecutive tiles of its list; item_off[pairs + 1] is the exclusive prefix sum of the pairs' item
// counts, written by ivfpq4_rscan_items_kernel in one workgroup before the scan, and workgroup w finds its pair as the last p
// with item_off[p] <= w by a bisection that is uniform over the workgroup.  A workgroup with nothing to scan returns before it
// touches LDS; the others copy their pair's table (M * 64 bytes) once.  One barrier.  Then a lane does what ivfpq4_scan_kernel's
// does at pos = off[probe] + i, and writes keys[q][seg[slot] + i], the t the plan assigned, so the selection and the stats are
// the plain handle's.  The run stays ivfpq_rscan_plan's (1 .. IPQ_RUN_MAX, above 1 only when the launch has more tiles than
// IPQ_GRID workgroups): a table copy is small here, but a longer run still saves copies and launches no fewer workgroups than
// fill the chip.
__global__ __launch_bounds__(IPQ_TILE) void ivfpq4_rscan_items_kernel(IvfBatch a, int s0, int ns, int run, uint32_t *item_off)
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

template <int PCH, bool VIS>
__global__ __launch_bounds__(IPQ_TILE) void ivfpq4_rscan_kernel(IvfBatch a, int s0, int ns, const float *tables, int M_rt, const uint8_t *lcodes,
                                                                int64_t n, const uint32_t *rows, int64_t nvis, const uint32_t *item_off, int run)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int M = PCH > 0 ? PCH * 32 : M_rt, P = PCH > 0 ? PCH * 16 : (M_rt + 1) / 2;
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
    const uint32_t Pq = gseg[a.np]; // (<= pmax: no key is written at or beyond it)
    const uint32_t t0 = gseg[slot], t1 = std::min(gseg[slot + 1], Pq); // (the plan's prefix sums: t0 <= t1 <= Pq always)
    const uint32_t len = t1 > t0 ? t1 - t0 : 0u;
    if ((uint64_t)tile * IPQ_TILE >= len) return; // (the whole workgroup: nothing waits at the barrier below)
    const int64_t l = a.probes[q * a.np + slot];
    const uint32_t base = l >= 0 && l < a.L.nlist ? a.L.off[l] : 0xffffffffu; // (a non-empty slot is a list of the handle)
    ipq4_table_to_lds(smem, tables + pair * M * PQ4_K, M, tid);
    __syncthreads();
    uint64_t *keys = a.keys + q * a.pmax + t0;
    for (; tile < tile_end; tile += tile_step) { // (tile_step <= IPQ_GRID, and the first tile past len ends the loop: no wrap)
        const uint64_t i = (uint64_t)tile * IPQ_TILE + tid;
        if (i >= len) {
            if ((uint64_t)tile * IPQ_TILE >= len) break; // (the whole workgroup)
            continue;                                    // (a lane past the end of the last tile)
        }
        keys[i] = ipq4_key<PCH, VIS>(a, smem, lcodes, (uint64_t)base + i, M, P, n, rows, nvis);
    }
}

template <int PCH, bool VIS>
static void launch_ivfpq4_rscan_m(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n,
                                  const IvfpqRscanPlan &plan, const uint32_t *item_off, const uint32_t *rows, int64_t nvis, hipStream_t s)
{
    const size_t shmem = (size_t)M * PQ4_K * sizeof(float); // (at most 64 KB: M <= PQ4_MAX_M)
    const int64_t pairs = (int64_t)a.nq * ns;
    const dim3 grid(plan.items ? (unsigned)plan.grid : (unsigned)pairs, plan.items ? 1u : (unsigned)plan.groups);
    hipLaunchKernelGGL((ivfpq4_rscan_kernel<PCH, VIS>), grid, dim3(IPQ_TILE), shmem, s, a, s0, ns, tables, M, lcodes, n, rows, nvis,
                       plan.items ? item_off : nullptr, plan.run);
}

template <bool VIS>
static void launch_ivfpq4_rscan_v(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n, int64_t maxlen,
                                  uint32_t *item_off, const uint32_t *rows, int64_t nvis, hipStream_t s)
{
    if (a.nq <= 0 || ns <= 0 || n <= 0 || s0 < 0 || s0 + ns > a.np) return;
    IvfpqRscanPlan plan = ivfpq_rscan_plan((int64_t)a.nq * ns, a.nq, a.pmax, maxlen);
    if (plan.items && !item_off) plan = IvfpqRscanPlan{false, ivfpq_rscan_groups((int64_t)a.nq * ns, maxlen), 0, 0};
    if (plan.items) hipLaunchKernelGGL(ivfpq4_rscan_items_kernel, dim3(1), dim3(IPQ_TILE), 0, s, a, s0, ns, plan.run, item_off);
    switch (ipq4_form(M, lcodes)) { // ivfpq4_scan_kernel's forms
    case 1: return launch_ivfpq4_rscan_m<1, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 2: return launch_ivfpq4_rscan_m<2, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 3: return launch_ivfpq4_rscan_m<3, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 4: return launch_ivfpq4_rscan_m<4, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 6: return launch_ivfpq4_rscan_m<6, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    case 0: return launch_ivfpq4_rscan_m<0, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    default: return launch_ivfpq4_rscan_m<-1, VIS>(a, s0, ns, tables, M, lcodes, n, plan, item_off, rows, nvis, s);
    }
}

void launch_ivfpq4_rscan(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n, int64_t maxlen,
                         uint32_t *item_off, hipStream_t s)
{
    launch_ivfpq4_rscan_v<false>(a, s0, ns, tables, M, lcodes, n, maxlen, item_off, nullptr, 0, s);
}

void launch_ivfpq4_rscan_visible(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n,
                                 int64_t maxlen, uint32_t *item_off, const uint32_t *rows, int64_t nvis, hipStream_t s)
{
    if (nvis <= 0) return; // (every seg is 0: no key is read)
    launch_ivfpq4_rscan_v<true>(a, s0, ns, tables, M, lcodes, n, maxlen, item_off, rows, nvis, s);
}

} // namespace lb
