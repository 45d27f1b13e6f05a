// kernels_ivfsq8_group.hip -- the list-major form of the IVF-SQ8 list scan (ivfsq8.hip decides which batches take it; semantics
// in include/longbow_gpu.h, lb_gpu_ivfsq8_search): the tile that scores 128 rows of a list against up to 64 of the queries that
// probe it on the i8 matrix cores.  The grouping of a batch's pairs by list is the IVF-Flat tiles' (kernels_ivf_group.hip:
// launch_ivf_group), and so are the work items; the keys are ivfsq8_scan_kernel's (kernels_ivfsq8.hip), bit for bit, and
// launch_ivfsq8_select runs behind either form.
//
// Why.  ivfsq8_scan_kernel stages a list once for every (query, probe slot) pair that probes it and scores it one lane a row
// with v_dot4_u32_u8.  The key is the exact integer S = sum (a - b)^2 over the codes, and integer sums leave the same bits in any
// order, so v_mfma_i32_32x32x32_i8 may form them, 32 rows and 32 queries an instruction, and a list's rows are read once for
// all 64 queries of a group.
//
// Signed bytes.  The matrix cores multiply signed bytes, so every real 16-byte piece of a row's and a query's code is shifted
// by 128 (^ 0x80808080) as it is staged.  The pad bytes inside a real piece are shifted on both sides too, which changes nothing:
// (x - 128) - (q - 128) = x - q byte for byte.  Pieces at or beyond `stride` stay zero on both sides.  So
// S = |x'|^2 + |q'|^2 - 2 x'.q' with no correction term.  Both norms are v_dot4_i32_i8 of the shifted pieces with themselves at
// staging, summed over a tile's chunks and then over the eight lanes that hold a row; nothing is stored beside the codes and
// qnorms is not read.
//
// Integer range.  stride <= 8,192 shifted bytes lie in [-128, 127]: |x'.q'| <= 8192 * 2^14 = 2^27, each norm is at most 2^27,
// |x'|^2 + |q'|^2 <= 2^28 and 2 x'.q' lies within +-2^28, so every intermediate stays inside int32; the result is
// S = sum (x - q)^2 <= 8192 * 65025 < 2^29.  There are no chains, no rounding and no fallback: one i32x16 accumulator a query
// column holds the total at every dimension, so a workgroup takes both columns of a group, 64 queries.
//
// The shape.  256 threads, four waves; a work item is a list and up to 64 of the pairs that probe it, and the workgroup walks the
// 128-row tiles blockIdx.x, blockIdx.x + gridDim.x, ... of the list, a wave owning 32 rows.  A stage is 128 bytes of every row and
// query: four K-steps of 32.  Thread t stages piece t % 8 of rows t / 8 + 32 i (i < 4) and of queries t / 8 + 32 j (j < JN), rows
// gathered by row number from codes + row * stride, into an LDS stage whose row stride is 144 bytes (36 dwords: the 16 rows
// that a ds_read_b128 serves at once start at banks 36 r mod 64, sixteen different multiples of 4, so their 64 dwords fall on 64
// different banks).  The next stage's global loads are held in
// registers while the current stage's MFMAs issue.  K-steps that are all padding are not issued.  A list entry at or beyond n
// reads row n - 1, as in the per-pair scan.
//
// The epilogue.  The S of one query column go through the freed stage as uint32 [query][row] at a stride of 129 words; then a
// wave takes a query and a lane a list position: keys[q pmax + seg + pos] = (S << 32) | row, 512 B a wave and store.
//
// The build (gfx950, -O3): 106 VGPRs, no AGPRs, no scratch, 28,928 B of LDS: four waves a SIMD, which is four workgroups a CU
// (the launch bound's; LDS alone would let five).
#include "lb_device.h"
#include "lb_ivfsq8.h"
#include "lb_list_scan.h"

#include <algorithm>

namespace lb {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int SQG_THREADS = 256;
constexpr int SQG_ROWS = 128;                       // rows per tile: 32 a wave
constexpr int SQG_COL = 32;                         // queries per column
constexpr int SQG_CK = 128;                         // bytes per row and query per stage: four K-steps of 32
constexpr int SQG_LD = SQG_CK + 16;                 // LDS row stride (bytes)
constexpr int SQG_PPR = SQG_CK / 16;                // 16-byte pieces per row per stage == lanes that share a row
constexpr int SQG_XPT = SQG_ROWS * SQG_PPR / SQG_THREADS; // row pieces per thread per stage (4); a query column is one each
constexpr int SQG_STAGE = (SQG_ROWS + IVF_GROUP_PAIRS) * SQG_LD; // 27,648 B
constexpr int SQG_TLD = SQG_ROWS + 1;               // words per query of the transposed S: odd
constexpr int SQG_SHIFT = (int)0x80808080u;         // uint8 -> the signed byte 128 below it, four at a time
static_assert(SQG_COL * SQG_PPR == SQG_THREADS && SQG_XPT * SQG_COL == SQG_ROWS, "a thread stages piece tid % 8 of row and query tid / 8 + 32 i");
static_assert(2 * SQG_COL == IVF_GROUP_PAIRS, "a group is two query columns");
static_assert(SQG_COL * SQG_TLD * 4 <= SQG_STAGE, "one query column's S fit the free stage");

// What a workgroup's item is, wave-uniform
struct Sq8GroupWork {
    uint32_t len;          // rows of the list
    const uint32_t *rmap;  // the list's rows, ascending
    const uint32_t *pairs; // the group's pairs
    int gn;                // pairs of the group, 1 .. 64
};

// the sum over the eight consecutive lanes that hold one row's pieces, in all of them
__device__ __forceinline__ int sqg_sum8(int v)
{
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v + __shfl_xor(v, 4);
}

// One held piece into its slot of the stage, shifted if it is real -> its share of the row's or query's |.'|^2
__device__ __forceinline__ int sqg_put(int8_t *slot, i32x4 v, bool real)
{
    if (real) v ^= i32x4{SQG_SHIFT, SQG_SHIFT, SQG_SHIFT, SQG_SHIFT};
    *reinterpret_cast<i32x4 *>(slot) = v;
    int t = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) t = __builtin_amdgcn_sdot4(v[j], v[j], t, false);
    return t;
}

// JN: query columns of 32 the group fills.  lnx[r]: |x'|^2 of row r of the tile; lqn[c]: |q'|^2 of the group's c-th pair's query;
// s_base[c]: where the keys of that pair start, -1 for a pair whose keys would leave its query's pmax.
template <int JN>
__device__ __forceinline__ void ivfsq8_tile_body(const IvfSq8Scan &s, const Sq8GroupWork &w, int8_t *lds, int *lnx, int *lqn, const int64_t *s_base)
{
    const IvfBatch &a = s.b;
    int8_t *lx = lds, *lq = lds + SQG_ROWS * SQG_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sp = tid & (SQG_PPR - 1), sr = tid / SQG_PPR; // staging: piece sp of row sr + 32 i of the tile, of query sr + 32 j of the group
    const int stride = s.stride;
    const int nchunks = (stride + SQG_CK - 1) / SQG_CK;
    const uint32_t ntiles = (w.len + SQG_ROWS - 1) / SQG_ROWS;
    const uint32_t last_row = (uint32_t)(s.n - 1);

    i32x4 px[SQG_XPT], pq[JN];
    uint32_t xrow[SQG_XPT], qoff[JN]; // (a batch's query codes hold fewer than 2^31 bytes)
    int nxp[SQG_XPT], nqp[JN];        // this thread's share of the norms of its rows of the tile, of its queries
#pragma unroll
    for (int j = 0; j < JN; j++) {
        qoff[j] = w.pairs[std::min(sr + SQG_COL * j, w.gn - 1)] / (uint32_t)a.np * (uint32_t)stride;
        nqp[j] = 0;
    }
    auto load_stage = [&](uint32_t tile, int c) {
        const int k = c * SQG_CK + sp * 16;
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < SQG_XPT; i++) {
                uint32_t pos = tile * SQG_ROWS + sr + SQG_COL * i;
                if (pos >= w.len) pos = w.len - 1; // (computed, never written)
                const uint32_t r = w.rmap[pos];
                xrow[i] = r < last_row ? r : last_row;
            }
        }
#pragma unroll
        for (int i = 0; i < SQG_XPT; i++) {
            px[i] = i32x4{0, 0, 0, 0};
            // (a plain load: other groups of the same list find the rows in L2 / MALL)
            if (k < stride) px[i] = *reinterpret_cast<const i32x4 *>(s.codes + (int64_t)xrow[i] * stride + k);
        }
#pragma unroll
        for (int j = 0; j < JN; j++) {
            pq[j] = i32x4{0, 0, 0, 0};
            if (k < stride) pq[j] = *reinterpret_cast<const i32x4 *>(s.qcodes + qoff[j] + k);
        }
    };
    // c: the chunk the held pieces are; first: of the first tile this workgroup walks (the queries' norms stay from it)
    auto write_stage = [&](int c, bool first) {
        const bool real = c * SQG_CK + sp * 16 < stride;
#pragma unroll
        for (int i = 0; i < SQG_XPT; i++) {
            const int t = sqg_put(&lx[(sr + SQG_COL * i) * SQG_LD + 16 * sp], px[i], real);
            nxp[i] = c == 0 ? t : nxp[i] + t;
        }
#pragma unroll
        for (int j = 0; j < JN; j++) {
            const int t = sqg_put(&lq[(sr + SQG_COL * j) * SQG_LD + 16 * sp], pq[j], real);
            if (first) nqp[j] += t;
        }
        if (c != nchunks - 1) return;
#pragma unroll
        for (int i = 0; i < SQG_XPT; i++) {
            const int t = sqg_sum8(nxp[i]);
            if (sp == 0) lnx[sr + SQG_COL * i] = t;
        }
        if (first) {
#pragma unroll
            for (int j = 0; j < JN; j++) {
                const int t = sqg_sum8(nqp[j]);
                if (sp == 0) lqn[sr + SQG_COL * j] = t;
            }
        }
    };

    // acc[j][e]: x'.q' of row 32 wave + (e & 3) + 8 (e >> 2) + 4 (lane >> 5) of the tile and query 32 j + (lane & 31) of the group
    i32x16 acc[JN];
    uint32_t tile = blockIdx.x;
    int c = 0;
    load_stage(tile, 0);
    write_stage(0, true);
    __syncthreads();
    while (true) {
        uint32_t ntile = tile;
        int nc = c + 1;
        if (nc == nchunks) {
            nc = 0;
            ntile = tile + gridDim.x;
        }
        const bool has_next = ntile < ntiles;
        if (has_next) load_stage(ntile, nc);
        if (c == 0) {
#pragma unroll
            for (int j = 0; j < JN; j++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[j][e] = 0;
        }
        // K-steps that are all padding are not issued
        const int ksteps = (std::min(stride - c * SQG_CK, SQG_CK) + 31) >> 5;
#pragma unroll
        for (int st = 0; st < SQG_CK / 32; st++) {
            if (st >= ksteps) break; // (uniform)
            const int off = st * 32 + (lane >> 5) * 16;
            const i32x4 fa = *reinterpret_cast<const i32x4 *>(&lx[(wave * 32 + (lane & 31)) * SQG_LD + off]);
#pragma unroll
            for (int j = 0; j < JN; j++) {
                const i32x4 fb = *reinterpret_cast<const i32x4 *>(&lq[(j * SQG_COL + (lane & 31)) * SQG_LD + off]);
                acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc[j], 0, 0, 0);
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (c == nchunks - 1) {
            // a column's S through the free stage, [query][row]; then a wave a query, a lane a list position
            uint32_t *lt = reinterpret_cast<uint32_t *>(lds);
            const uint32_t pos0 = tile * SQG_ROWS + lane, pos1 = pos0 + 64;
            const uint32_t row0 = pos0 < w.len ? w.rmap[pos0] : 0u, row1 = pos1 < w.len ? w.rmap[pos1] : 0u;
#pragma unroll
            for (int j = 0; j < JN; j++) {
                const int rl0 = wave * 32 + 4 * (lane >> 5);
                const int qn = lqn[j * SQG_COL + (lane & 31)];
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int rl = rl0 + (e & 3) + 8 * (e >> 2);
                    lt[(lane & 31) * SQG_TLD + rl] = (uint32_t)(lnx[rl] + qn - 2 * acc[j][e]); // 0 <= S < 2^29 (the bounds above)
                }
                __syncthreads();
                const int nj = std::min(w.gn - j * SQG_COL, SQG_COL);
                for (int jq = wave; jq < nj; jq += SQG_THREADS / 64) {
                    const int64_t base = s_base[j * SQG_COL + jq];
                    if (base < 0) continue;
                    if (pos0 < w.len) a.keys[base + pos0] = ((uint64_t)lt[jq * SQG_TLD + lane] << 32) | row0;
                    if (pos1 < w.len) a.keys[base + pos1] = ((uint64_t)lt[jq * SQG_TLD + lane + 64] << 32) | row1;
                }
                __syncthreads(); // the stage is free again
            }
        }
        if (!has_next) break;
        write_stage(nc, ntile == blockIdx.x); // (the first tile's later chunks complete the queries' norms)
        __syncthreads();
        tile = ntile;
        c = nc;
    }
}

// The item is blockIdx.y + blockIdx.z gridDim.y.  LDS: the stage (27,648 B), the tile's row norms (512 B), the group's query
// norms (256 B) and key bases (512 B).
__global__ __launch_bounds__(SQG_THREADS, 4) void ivfsq8_scan_tile_kernel(IvfSq8Scan s, IvfGroups g)
{
    __shared__ __attribute__((aligned(16))) int8_t lds[SQG_STAGE];
    __shared__ int lnx[SQG_ROWS];
    __shared__ int lqn[IVF_GROUP_PAIRS];
    __shared__ int64_t s_base[IVF_GROUP_PAIRS];
    const IvfBatch &a = s.b;
    const uint32_t item = blockIdx.y + blockIdx.z * gridDim.y;
    if (item >= g.nitems[0]) return;
    const uint2 it = g.items[item]; // (list, first pair): the list is below nlist and has rows
    const uint32_t off = a.L.off[it.x];
    Sq8GroupWork w;
    w.len = a.L.off[it.x + 1] - off;
    if ((uint64_t)blockIdx.x * SQG_ROWS >= w.len) return;
    w.rmap = a.L.rows + off;
    w.pairs = g.gpairs + it.y;
    w.gn = (int)std::min<uint32_t>(g.goff[it.x + 1] - it.y, IVF_GROUP_PAIRS);
    if ((int)threadIdx.x < w.gn) {
        const uint32_t pair = w.pairs[threadIdx.x];
        const uint32_t q = pair / (uint32_t)a.np, p = pair % (uint32_t)a.np;
        const uint32_t seg = a.seg[(int64_t)q * (a.np + 1) + p];
        // never refused with distinct probes: the keys of a query stay inside its pmax
        s_base[threadIdx.x] = (int64_t)seg + w.len > a.pmax ? -1 : (int64_t)q * a.pmax + seg;
    }
    // (the body's first barrier comes before any read of s_base)
    if (w.gn <= SQG_COL) ivfsq8_tile_body<1>(s, w, lds, lnx, lqn, s_base); // uniform: an empty query column costs nothing
    else ivfsq8_tile_body<2>(s, w, lds, lnx, lqn, s_base);
}

} // namespace

hipError_t launch_ivfsq8_scan_tile(const IvfSq8Scan &a, const IvfGroups &g, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.b.nq * a.b.np;
    if (pairs <= 0 || maxlen <= 0 || a.n <= 0) return hipSuccess;
    const hipError_t e = launch_ivf_group(a.b, g, s);
    if (e != hipSuccess) return e;
    const int64_t items = ivf_group_max_items(pairs, a.b.L.nlist), tiles = (maxlen + SQG_ROWS - 1) / SQG_ROWS;
    const unsigned gy = (unsigned)std::min<int64_t>(items, IVF_PAIRS_Y); // items <= 1024 * 65536 / 64 + 65536: z stays below 65536
    const dim3 grid((unsigned)list_scan_gx(items, tiles), gy, (unsigned)((items + gy - 1) / gy));
    hipLaunchKernelGGL(ivfsq8_scan_tile_kernel, grid, dim3(SQG_THREADS), 0, s, a, g);
    return hipSuccess;
}

} // namespace lb
