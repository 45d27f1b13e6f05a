// kernels_ivf_i8_group.hip -- the list-major form of the IVF-Flat list scan over int8 rows (ivf.hip decides which batches take
// it; semantics in include/longbow_gpu.h, lb_gpu_ivf_search): the tile that scores 128 rows of a list against up to 64 of the
// queries that probe it on the i8 matrix cores.  The grouping of a batch's pairs by list is the float32 tile's
// (kernels_ivf_group.hip: launch_ivf_group), and so are the work items, the grid and the walk.
//
// Why.  ivf_scan_i8_kernel (kernels_ivf_i8.hip) stages a list once for every (query, probe slot) pair that probes it and
// scores it one lane a row with v_dot4_i32_i8.  On the staged path x.q is an exact int32 and S = |x|^2 + |q|^2 - 2 x.q is
// rounded once, so any summation order leaves the same bits: v_mfma_i32_32x32x32_i8 computes x.q of 32 rows and 32 queries an
// instruction, as the flat int8 index's batched pass does (kernels_i8.hip: mfma_i8_kernel, whose operand and C/D lane maps
// these are).
//
// The tile.  A 256-thread workgroup takes one item (list, group of at most 64 pairs) and walks the list's 128-row tiles
// blockIdx.x, blockIdx.x + gridDim.x, ..., a tile in chunks of 128 bytes a row: one LDS stage [128 row chunks | 64 query chunks]
// of 16-byte pieces at a 144-byte stride (conflict-free ds_read_b128 fragment reads), zero beyond D, so that the 32-byte K-step
// is padded when D % 32 == 16; a K-step that is all padding is not issued.  The next stage's global loads are held in registers
// while the current one feeds the matrix cores, wrapping from a tile's last chunk to the next tile's first.  Wave w owns rows
// 32 w .. 32 w + 31 against the JN in {1, 2} query columns of 32 that hold a pair of the group: one row fragment is read and fed
// to both columns' accumulators (i32x16 each).  JN is uniform over the workgroup and a template argument of the body.
//
// Norms (L2), with no stored array.  A thread takes v_dot4_i32_i8 of every 16-byte row piece it has loaded with itself as it
// writes the piece to LDS, keeps the sum over the chunks of the tile, and at the tile's last chunk the eight lanes that hold one
// row's pieces add their sums across lanes; one of them leaves |x|^2 in LDS for the epilogue.  |q|^2 of the group's queries
// comes the same way from the query pieces of the first tile the workgroup walks, and stays.
//
// The keys.  The epilogue is ivf_scan_i8_kernel's finish, bit for bit: L2 (float)sqrt((double)(float)(xn + qn - 2 dot)), dot
// -(float)dot.  The C/D map gives a lane one query and 16 scattered rows, so the distances of one query column go through the
// free stage transposed ([query][row], 129 floats a query: 16.5 KB of the stage's 27), a column at a time, and wave w then
// writes queries w, w + 4, ... of the column, a lane a list position: a wave's stores for one query are consecutive entries of
// keys[q pmax + seg[q][p] + pos].  Rows beyond the list's length are computed and never written.
// No FMA contraction here.
#include "lb_device.h"
#include "lb_ivf_i8.h"
#include "lb_list_scan.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int I8G_THREADS = 256;
constexpr int I8G_ROWS = 128;                       // rows per tile: 32 a wave
constexpr int I8G_COL = 32;                         // queries per column
constexpr int I8G_CK = 128;                         // bytes per row and query per stage: four K-steps of 32
constexpr int I8G_LD = I8G_CK + 16;                 // LDS row stride (bytes): MF_LD's
constexpr int I8G_PPR = I8G_CK / 16;                // 16-byte pieces per row per stage == lanes that share a row
constexpr int I8G_XPT = I8G_ROWS * I8G_PPR / I8G_THREADS; // row pieces per thread per stage (4); a query column is one each
constexpr int I8G_STAGE = (I8G_ROWS + IVF_GROUP_PAIRS) * I8G_LD; // 27,648 B
constexpr int I8G_TLD = I8G_ROWS + 1;               // floats per query of the transposed distances
static_assert(I8G_COL * I8G_PPR == I8G_THREADS && I8G_XPT * I8G_COL == I8G_ROWS, "a thread stages piece tid % 8 of row and query tid / 8 + 32 i");
static_assert(I8G_COL * I8G_TLD * 4 <= I8G_STAGE, "one query column's distances fit the free stage");

// What a workgroup's item is, wave-uniform
struct I8GroupWork {
    uint32_t len;          // rows of the list
    const uint32_t *rmap;  // the list's rows, ascending
    const uint32_t *pairs; // the group's pairs
    int gn;                // pairs of the group, 1 .. 64
};

__device__ __forceinline__ int i8g_sq(const i32x4 v, int s)
{
    s = __builtin_amdgcn_sdot4(v.x, v.x, s, false);
    s = __builtin_amdgcn_sdot4(v.y, v.y, s, false);
    s = __builtin_amdgcn_sdot4(v.z, v.z, s, false);
    return __builtin_amdgcn_sdot4(v.w, v.w, s, false);
}
// the sum over the eight consecutive lanes that hold one row's pieces, in all of them
__device__ __forceinline__ int i8g_sum8(int v)
{
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v + __shfl_xor(v, 4);
}

// JN: query columns of 32 that hold a pair of the group.  lnx[r]: |x|^2 of row r of the tile; lqn[j]: |q|^2 of the group's j-th
// pair's query; s_base[j]: where the keys of that pair start, -1 for a pair whose keys would leave its query's pmax.
template <int METRIC, int JN>
__device__ __forceinline__ void ivf_i8_tile_body(const IvfI8Scan &s, const I8GroupWork &w, int8_t *lds, int *lnx, int *lqn, const int64_t *s_base)
{
    const IvfBatch &a = s.b;
    int8_t *lx = lds, *lq = lds + I8G_ROWS * I8G_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sp = tid & (I8G_PPR - 1), sr = tid / I8G_PPR; // staging: piece sp of row sr + 32 i of the tile, of query sr + 32 j of the group
    const int D = a.D;
    const int nchunks = (D + I8G_CK - 1) / I8G_CK;
    const uint32_t ntiles = (w.len + I8G_ROWS - 1) / I8G_ROWS;

    i32x4 px[I8G_XPT], pq[JN];
    uint32_t xrow[I8G_XPT], qoff[JN]; // (a batch's queries hold fewer than 2^31 bytes)
    int nxp[I8G_XPT], nqp[JN];        // L2: this thread's share of |x|^2 of its rows of the tile, of |q|^2 of its queries
#pragma unroll
    for (int j = 0; j < JN; j++) {
        qoff[j] = w.pairs[std::min(sr + I8G_COL * j, w.gn - 1)] / (uint32_t)a.np * (uint32_t)D;
        nqp[j] = 0;
    }
    auto load_stage = [&](uint32_t tile, int c) {
        const int k = c * I8G_CK + sp * 16;
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < I8G_XPT; i++) {
                uint32_t pos = tile * I8G_ROWS + sr + I8G_COL * i;
                if (pos >= w.len) pos = w.len - 1; // (computed, never written)
                xrow[i] = w.rmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < I8G_XPT; i++) {
            px[i] = i32x4{0, 0, 0, 0};
            // (a plain load: other groups of the same list find the rows in L2 / MALL)
            if (k < D) px[i] = *reinterpret_cast<const i32x4 *>(s.X + (int64_t)xrow[i] * D + k);
        }
#pragma unroll
        for (int j = 0; j < JN; j++) {
            pq[j] = i32x4{0, 0, 0, 0};
            if (k < D) pq[j] = *reinterpret_cast<const i32x4 *>(s.Q + qoff[j] + k);
        }
    };
    // c: the chunk the held pieces are; first: of the first tile this workgroup walks
    auto write_stage = [&](int c, bool first) {
#pragma unroll
        for (int i = 0; i < I8G_XPT; i++) *reinterpret_cast<i32x4 *>(&lx[(sr + I8G_COL * i) * I8G_LD + sp * 16]) = px[i];
#pragma unroll
        for (int j = 0; j < JN; j++) *reinterpret_cast<i32x4 *>(&lq[(sr + I8G_COL * j) * I8G_LD + sp * 16]) = pq[j];
        if (METRIC != METRIC_L2) return;
#pragma unroll
        for (int i = 0; i < I8G_XPT; i++) nxp[i] = i8g_sq(px[i], c == 0 ? 0 : nxp[i]);
        if (first) {
#pragma unroll
            for (int j = 0; j < JN; j++) nqp[j] = i8g_sq(pq[j], nqp[j]);
        }
        if (c != nchunks - 1) return;
#pragma unroll
        for (int i = 0; i < I8G_XPT; i++) {
            const int t = i8g_sum8(nxp[i]);
            if (sp == 0) lnx[sr + I8G_COL * i] = t;
        }
        if (first) {
#pragma unroll
            for (int j = 0; j < JN; j++) {
                const int t = i8g_sum8(nqp[j]);
                if (sp == 0) lqn[sr + I8G_COL * j] = t;
            }
        }
    };

    i32x16 acc[JN]; // [column j]: x.q of row 32 wave + (e & 3) + 8 (e >> 2) + 4 (lane >> 5) and query 32 j + (lane & 31)
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
        const int ksteps = (std::min(D - c * I8G_CK, I8G_CK) + 31) >> 5;
#pragma unroll
        for (int st = 0; st < I8G_CK / 32; st++) {
            if (st >= ksteps) break; // (uniform: K-steps that are all padding)
            const int off = st * 32 + (lane >> 5) * 16;
            const i32x4 fa = *reinterpret_cast<const i32x4 *>(&lx[(wave * 32 + (lane & 31)) * I8G_LD + off]);
#pragma unroll
            for (int j = 0; j < JN; j++) {
                const i32x4 fb = *reinterpret_cast<const i32x4 *>(&lq[(j * I8G_COL + (lane & 31)) * I8G_LD + off]);
                acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc[j], 0, 0, 0);
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (c == nchunks - 1) {
            // a column's distances through the free stage, [query][row]; then a wave a query, a lane a list position
            float *lt = reinterpret_cast<float *>(lds);
            const uint32_t pos0 = tile * I8G_ROWS + lane, pos1 = pos0 + 64;
            const uint32_t row0 = pos0 < w.len ? w.rmap[pos0] : 0u, row1 = pos1 < w.len ? w.rmap[pos1] : 0u;
#pragma unroll
            for (int j = 0; j < JN; j++) {
                const int qn = METRIC == METRIC_L2 ? lqn[j * I8G_COL + (lane & 31)] : 0;
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int rl = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    const int dot = acc[j][e];
                    float dist;
                    // L2: S <= 8192 * 65025 < 2^31, converted once to f32, sqrt correctly rounded; dot: |x.q| <= 2^24, exact
                    if (METRIC == METRIC_L2) dist = (float)sqrt((double)(float)(lnx[rl] + qn - 2 * dot));
                    else dist = -(float)dot;
                    lt[(lane & 31) * I8G_TLD + rl] = dist;
                }
                __syncthreads();
                const int nj = std::min(w.gn - j * I8G_COL, I8G_COL);
                for (int jq = wave; jq < nj; jq += I8G_THREADS / 64) {
                    const int64_t base = s_base[j * I8G_COL + jq];
                    if (base < 0) continue;
                    if (pos0 < w.len) a.keys[base + pos0] = pack_entry(lt[jq * I8G_TLD + lane], row0);
                    if (pos1 < w.len) a.keys[base + pos1] = pack_entry(lt[jq * I8G_TLD + lane + 64], row1);
                }
                __syncthreads(); // the stage is free again
            }
        }
        if (!has_next) break;
        write_stage(nc, ntile == blockIdx.x);
        __syncthreads();
        tile = ntile;
        c = nc;
    }
}

// ivf_scan_i8_staged holds.  LDS: the stage (27,648 B), the tile's row norms (512 B), the group's query norms (256 B) and key
// bases (512 B).
template <int METRIC>
__global__ __launch_bounds__(I8G_THREADS, 4) void ivf_scan_i8_tile_kernel(IvfI8Scan s, IvfGroups g)
{
    __shared__ __attribute__((aligned(16))) int8_t lds[I8G_STAGE];
    __shared__ int lnx[I8G_ROWS];
    __shared__ int lqn[IVF_GROUP_PAIRS];
    __shared__ int64_t s_base[IVF_GROUP_PAIRS];
    const IvfBatch &a = s.b;
    const uint32_t item = blockIdx.y + blockIdx.z * gridDim.y;
    if (item >= g.nitems[0]) return;
    const uint2 it = g.items[item]; // (list, first pair): the list is below nlist and has rows
    const uint32_t off = a.L.off[it.x];
    I8GroupWork w;
    w.len = a.L.off[it.x + 1] - off;
    if ((uint64_t)blockIdx.x * I8G_ROWS >= w.len) return;
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
    if (w.gn <= I8G_COL) ivf_i8_tile_body<METRIC, 1>(s, w, lds, lnx, lqn, s_base); // uniform: an empty query column costs nothing
    else ivf_i8_tile_body<METRIC, 2>(s, w, lds, lnx, lqn, s_base);
}

hipError_t launch_ivf_scan_i8_tile(int metric, const IvfI8Scan &a, const IvfGroups &g, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.b.nq * a.b.np;
    if (pairs <= 0 || maxlen <= 0) return hipSuccess;
    const hipError_t e = launch_ivf_group(a.b, g, s);
    if (e != hipSuccess) return e;
    const int64_t items = ivf_group_max_items(pairs, a.b.L.nlist), tiles = (maxlen + I8G_ROWS - 1) / I8G_ROWS;
    const unsigned gy = (unsigned)std::min<int64_t>(items, IVF_PAIRS_Y);
    const dim3 grid((unsigned)list_scan_gx(items, tiles), gy, (unsigned)((items + gy - 1) / gy));
    if (metric == METRIC_L2) hipLaunchKernelGGL((ivf_scan_i8_tile_kernel<METRIC_L2>), grid, dim3(I8G_THREADS), 0, s, a, g);
    else hipLaunchKernelGGL((ivf_scan_i8_tile_kernel<METRIC_DOT>), grid, dim3(I8G_THREADS), 0, s, a, g);
    return hipSuccess;
}

} // namespace lb
