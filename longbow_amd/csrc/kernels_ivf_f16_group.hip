// kernels_ivf_f16_group.hip -- the list-major form of the IVF-Flat list scan over float16 rows (ivf.hip decides which batches
// take it; semantics in include/longbow_gpu.h, lb_gpu_ivf_search): the tile that scores 64 rows of a list against up to 64 of
// the queries that probe it.  The grouping of a batch's (query, probe slot) pairs by list is the float32 tile's
// (launch_ivf_group, kernels_ivf_group.hip), and so are the work items, the grid and the lane map.
//
// Why.  ivf_scan_f16_kernel (kernels_ivf_f16.hip) stages a list once for every pair that probes it.  Here a staged element of a
// row meets up to 64 queries and a staged element of a query 64 rows, as in ivf_scan_tile_kernel; the rows cross L2, the staging
// registers and LDS as fp16, half the float32 tile's bytes at each of the three.
//
// Arithmetic.  ivf_scan_f16_kernel's: an fp16 element is widened to f32 as a lane reads it from LDS (exact), four elements enter
// the pair's Acc<ORDER> through add4_pair<METRIC>(q, x) in ascending dimension, under cosine add4_sq of the row first, and the
// finish is exact_distance<METRIC>(., D, false).  A key equals that kernel's key bit for bit and lands where it puts it:
// keys[q pmax + seg[q][p] + pos].  No matrix instruction: an fp16 MFMA sums in another order.
//
// Work.  A 256-thread workgroup takes one item (list, first pair of a group of at most 64 pairs) and walks the list's 64-row
// tiles blockIdx.x, blockIdx.x + gridDim.x, ..., a tile in chunks of IHG_DK elements: one LDS stage [64 row chunks fp16 | 64 query
// chunks f32], the next stage's global loads held in registers meanwhile, wrapping from a tile's last chunk to the next tile's
// first.  Lane (ty, tx) = (tid / 16, tid % 16) keeps the 4 x JN pairs of rows ty + 16 i and queries tx + 16 j; JN = ceil(group
// size / 16) is uniform over the workgroup and a template argument of the body.  Per 16-byte piece of a row a lane reads the
// raw eight halves of its four rows (four ds_read_b128), then widens and consumes the low four elements of every row against the
// JN query vectors of those four dimensions, then the high four: beside a row's raw f16x8 one f32x4 of it is live at a time.
// Every row element is widened by each of the 16 lanes that share it: 32 conversions a lane per eight dimensions, beside
// 4 JN 8 3 arithmetic operations under L2 (8 % of them at JN = 4, 33 % at JN = 1).
//
// LDS banks (4-byte banks; stated for 32 banks served a quarter-wave of b128 accesses at a time, and for 64 served sixteen
// lanes at a time).  Row stride IHG_LDX = IHG_DK + 8 = 72 halves = 36 dwords (4 mod 32, 36 mod 64); query stride IHG_LDQ =
// IHG_DK + 4 = 68 floats, the float32 tile's.
//   the staging write: thread tid writes piece tid % 8 of rows tid / 8 + 32 i, so eight consecutive lanes write one row's 128
//     consecutive bytes: 32 different banks, conflict-free at any stride that keeps the pieces 16-byte aligned.  If sixteen
//     lanes are served at once over 64 banks they are rows r and r + 1, 36 dwords apart: banks b .. b + 31 and b + 36 .. b + 67,
//     which meet on four banks of the 64.  A stride of 32 mod 64 dwords would part them and break the read below; 36 is kept.
//   the consume read: the 16 tx lanes of a row read one address (a broadcast), so a wave reads four addresses: piece g of rows
//     ty0 .. ty0 + 3, 16 bytes each.  At 36 dwords a row they start at banks const + 0, 36, 8, 44 (mod 64) or const + 0, 4, 8,
//     12 (mod 32): sixteen different banks, conflict-free under either count.  ivf_scan_f16_kernel needs its 128 + 8 halves so
//     that 64 lanes reading 64 different rows spread over all banks, eight rows a pass (8 x 4 dwords = 32); here only four
//     rows are read at once, and any stride whose dword count is 4, 8 or 12 mod 16 would do (not 0 mod 16: rows r and r + 2
//     would meet).  8 halves is the smallest pad that keeps the pieces 16-byte aligned, and it gives 4.
//   the query read: lane tx reads query tx + 16 j, the four ty of a wave the same address: sixteen addresses 68 dwords apart,
//     banks 4 tx + const: 64 different banks, or twice eight lanes on 32 different banks.  Conflict-free, as in the float32 tile.
//   the transposed keys go through the free query stage at the float32 tile's stride 68, conflict-free both ways as there.
//
// IHG_DK = 64.  The body is written for 64 or 128; at 128 the cosine SEQ instantiation spills at three workgroups a CU (DESIGN
// 3.30 has both build reports), so 64 it is.
// No FMA contraction here.
#include "lb_device.h"
#include "lb_exact.h"
#include "lb_ivf_f16.h"
#include "lb_list_scan.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

constexpr int IHG_THREADS = 256;
constexpr int IHG_ROWS = 64;          // rows per tile
constexpr int IHG_DK = 64;            // elements per row and per query per stage
constexpr int IHG_LDX = IHG_DK + 8;   // padded LDS row stride (halves)
constexpr int IHG_LDQ = IHG_DK + 4;   // padded LDS query stride (floats)
constexpr int IHG_LDT = 68;           // stride of the transposed distances (floats): the float32 tile's IG_LD
constexpr int IHG_PER = 4;            // rows per lane; query columns per lane at most
constexpr int IHG_XPR = IHG_DK / 8;   // 16-byte pieces per row chunk
constexpr int IHG_XN = IHG_ROWS * IHG_XPR / IHG_THREADS; // row pieces a thread stages
constexpr int IHG_XRS = IHG_THREADS / IHG_XPR;           // rows between a thread's row pieces
constexpr int IHG_QN = IHG_DK / 64;   // pieces of a query's chunk a thread stages: tx, tx + 16, ...
static_assert(IHG_DK == 64 || IHG_DK == 128, "the stage is 64 or 128 elements");
static_assert(IHG_ROWS * IHG_LDT <= IVF_GROUP_PAIRS * IHG_LDQ, "the transposed distances fit the query stage");

// What a workgroup's item is, wave-uniform
struct F16GroupWork {
    uint32_t len;          // rows of the list
    const uint32_t *rmap;  // the list's rows, ascending
    const uint32_t *pairs; // the group's pairs
    int gn;                // pairs of the group, 1 .. 64
};

// JN: query columns of 16 that hold a pair of the group.  s_base[j]: where the keys of the group's j-th pair start, -1 for a
// pair whose keys would leave its query's pmax (ivf_list_work's guard).  s_na[j]: ||q||^2 of that pair's query (cosine), read
// at a tile's finish and so not held in registers across the chunks.
template <int METRIC, int ORDER, int JN>
__device__ __forceinline__ void ivf_f16_tile_body(const IvfF16Scan &s, const F16GroupWork &w, _Float16 *lx, float *lq, const int64_t *s_base,
                                                  const float *s_na)
{
    const IvfBatch &a = s.b;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wave = tid >> 6;
    const int xp = tid % IHG_XPR, xr = tid / IHG_XPR; // staging: piece xp of rows xr + IHG_XRS i (at 128: piece tx of rows ty + 16 i)
    const int D = a.D;
    const int nchunks = (D + IHG_DK - 1) / IHG_DK;
    const uint32_t ntiles = (w.len + IHG_ROWS - 1) / IHG_ROWS;

    f16x8 sx[IHG_XN];
    f32x4 sq[JN][IHG_QN]; // pieces tx + 16 h of query ty + 16 j of the group
    // qoff: byte offsets into the batch's queries (at most 1,024 x LB_MAX_DIM floats, 2^25 bytes): a 32-bit offset beside the
    // uniform base, where a pointer per query column would hold eight registers across the chunks
    uint32_t xrow[IHG_XN], qoff[JN];
    const char *qbase = reinterpret_cast<const char *>(a.Q);
#pragma unroll
    for (int j = 0; j < JN; j++) qoff[j] = w.pairs[std::min(ty + 16 * j, w.gn - 1)] / (uint32_t)a.np * (uint32_t)D * 4u;
    auto load_stage = [&](uint32_t tile, int c) {
        int kx = c * IHG_DK + xp * 8;
        if (kx > D - 8) kx = D - 8; // (a piece past D is never consumed)
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < IHG_XN; i++) {
                uint32_t pos = tile * IHG_ROWS + xr + IHG_XRS * i;
                if (pos >= w.len) pos = w.len - 1; // (computed, never written)
                xrow[i] = w.rmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < IHG_XN; i++) sx[i] = *reinterpret_cast<const f16x8 *>(s.X + (int64_t)xrow[i] * D + kx);
#pragma unroll
        for (int h = 0; h < IHG_QN; h++) {
            int kq = c * IHG_DK + (tx + 16 * h) * 4;
            if (kq > D - 4) kq = D - 4;
#pragma unroll
            for (int j = 0; j < JN; j++) sq[j][h] = *reinterpret_cast<const f32x4 *>(qbase + (qoff[j] + (uint32_t)kq * 4u));
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < IHG_XN; i++) *reinterpret_cast<f16x8 *>(&lx[(xr + IHG_XRS * i) * IHG_LDX + xp * 8]) = sx[i];
#pragma unroll
        for (int j = 0; j < JN; j++)
#pragma unroll
            for (int h = 0; h < IHG_QN; h++) *reinterpret_cast<f32x4 *>(&lq[(ty + 16 * j) * IHG_LDQ + (tx + 16 * h) * 4]) = sq[j][h];
    };

    Acc<ORDER> acc[IHG_PER][JN]; // [row ty + 16 i][query tx + 16 j]: L2 sum (q-x)^2 ; cos/dot sum q*x
    Acc<ORDER> nb[IHG_PER];      // cos: sum x*x of row ty + 16 i

    uint32_t tile = blockIdx.x;
    int c = 0;
    load_stage(tile, 0);
    write_stage();
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
            for (int i = 0; i < IHG_PER; i++) {
                nb[i].zero();
#pragma unroll
                for (int j = 0; j < JN; j++) acc[i][j].zero();
            }
        }
        const int d0 = c * IHG_DK;
        const int npieces = (min(D, d0 + IHG_DK) - d0) >> 3;
#pragma unroll 1
        for (int g = 0; g < npieces; g++) { // (a piece is two of the float32 tile's groups: its loop is unrolled by two)
            f16x8 xh[IHG_PER];
#pragma unroll
            for (int i = 0; i < IHG_PER; i++) xh[i] = *reinterpret_cast<const f16x8 *>(&lx[(ty + 16 * i) * IHG_LDX + g * 8]);
#pragma unroll
            for (int h = 0; h < 2; h++) { // the low four elements of the piece, then the high four
                f32x4 qv[JN];
#pragma unroll
                for (int j = 0; j < JN; j++) qv[j] = *reinterpret_cast<const f32x4 *>(&lq[(tx + 16 * j) * IHG_LDQ + g * 8 + h * 4]);
#pragma unroll
                for (int i = 0; i < IHG_PER; i++) {
                    const f32x4 xv = {(float)xh[i][4 * h], (float)xh[i][4 * h + 1], (float)xh[i][4 * h + 2], (float)xh[i][4 * h + 3]};
                    if (METRIC == METRIC_COS) nb[i].add4_sq(xv);
#pragma unroll
                    for (int j = 0; j < JN; j++) acc[i][j].template add4_pair<METRIC>(qv[j], xv);
                    // a row's four elements are widened when the row before is consumed, not all of a piece's 32 ahead of it
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (c == nchunks - 1) {
            // the tile's distances through the free query stage, [query][row]; then a wave a query, a lane a list position
            float *lt = lq;
#pragma unroll
            for (int i = 0; i < IHG_PER; i++) {
                const float nbt = nb[i].total();
#pragma unroll
                for (int j = 0; j < JN; j++)
                    lt[(tx + 16 * j) * IHG_LDT + ty + 16 * i] = exact_distance<METRIC>(acc[i][j].total(), nbt, s_na[tx + 16 * j], D, false);
            }
            __syncthreads();
            const uint32_t pos = tile * IHG_ROWS + lane;
            if (pos < w.len) {
                const uint32_t row = w.rmap[pos];
                for (int j = wave; j < w.gn; j += IHG_THREADS / 64) {
                    const int64_t base = s_base[j];
                    if (base >= 0) a.keys[base + pos] = pack_entry(lt[j * IHG_LDT + lane], row);
                }
            }
            __syncthreads(); // the stage is free again
        }
        if (!has_next) break;
        write_stage();
        __syncthreads();
        tile = ntile;
        c = nc;
    }
}

// D % 8 == 0, X and Q 16-byte aligned (ivf_scan_f16_staged).  LDS: the rows' stage, the queries' stage and the group's key bases.
template <int METRIC, int ORDER>
__global__ __launch_bounds__(IHG_THREADS, ORDER == ORDER_SEQ ? 3 : 2) void ivf_scan_f16_tile_kernel(IvfF16Scan s, IvfGroups g)
{
    __shared__ __attribute__((aligned(16))) _Float16 lds_x[IHG_ROWS * IHG_LDX];
    __shared__ __attribute__((aligned(16))) float lds_q[IVF_GROUP_PAIRS * IHG_LDQ];
    __shared__ int64_t s_base[IVF_GROUP_PAIRS];
    __shared__ float s_na[IVF_GROUP_PAIRS];
    const IvfBatch &a = s.b;
    const uint32_t item = blockIdx.y + blockIdx.z * gridDim.y;
    if (item >= g.nitems[0]) return;
    const uint2 it = g.items[item]; // (list, first pair): the list is below nlist and has rows
    const uint32_t off = a.L.off[it.x];
    F16GroupWork w;
    w.len = a.L.off[it.x + 1] - off;
    if ((uint64_t)blockIdx.x * IHG_ROWS >= w.len) return;
    w.rmap = a.L.rows + off;
    w.pairs = g.gpairs + it.y;
    w.gn = (int)std::min<uint32_t>(g.goff[it.x + 1] - it.y, IVF_GROUP_PAIRS);
    if ((int)threadIdx.x < w.gn) {
        const uint32_t pair = w.pairs[threadIdx.x];
        const uint32_t q = pair / (uint32_t)a.np, p = pair % (uint32_t)a.np;
        const uint32_t seg = a.seg[(int64_t)q * (a.np + 1) + p];
        // never refused with distinct probes: the keys of a query stay inside its pmax
        s_base[threadIdx.x] = (int64_t)seg + w.len > a.pmax ? -1 : (int64_t)q * a.pmax + seg;
        s_na[threadIdx.x] = METRIC == METRIC_COS ? a.qna[q] : 0.f;
    } else if (threadIdx.x < IVF_GROUP_PAIRS) s_na[threadIdx.x] = 0.f; // (a column's queries past the group: computed, never written)
    // (the body's first barrier comes before any read of s_base and s_na)
    switch ((w.gn + 15) >> 4) { // uniform over the workgroup: whole empty query columns cost nothing
    case 1: ivf_f16_tile_body<METRIC, ORDER, 1>(s, w, lds_x, lds_q, s_base, s_na); break;
    case 2: ivf_f16_tile_body<METRIC, ORDER, 2>(s, w, lds_x, lds_q, s_base, s_na); break;
    case 3: ivf_f16_tile_body<METRIC, ORDER, 3>(s, w, lds_x, lds_q, s_base, s_na); break;
    default: ivf_f16_tile_body<METRIC, ORDER, 4>(s, w, lds_x, lds_q, s_base, s_na); break;
    }
}

hipError_t launch_ivf_scan_f16_tile(int metric, int order, const IvfF16Scan &a, const IvfGroups &g, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.b.nq * a.b.np;
    if (pairs <= 0 || maxlen <= 0) return hipSuccess;
    const hipError_t e = launch_ivf_group(a.b, g, s);
    if (e != hipSuccess) return e;
    const int64_t items = ivf_group_max_items(pairs, a.b.L.nlist), tiles = (maxlen + IHG_ROWS - 1) / IHG_ROWS;
    const unsigned gy = (unsigned)std::min<int64_t>(items, IVF_PAIRS_Y);
    const dim3 grid((unsigned)list_scan_gx(items, tiles), gy, (unsigned)((items + gy - 1) / gy));
    with_metric_order(metric, order, [&](auto m, auto o) {
        hipLaunchKernelGGL((ivf_scan_f16_tile_kernel<decltype(m)::value, decltype(o)::value>), grid, dim3(IHG_THREADS), 0, s, a, g);
    });
    return hipSuccess;
}

} // namespace lb
