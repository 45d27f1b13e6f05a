// kernels_ivf_u8_group.hip -- the list-major form of the IVF-Flat list scan over uint8 rows (ivf.hip decides which batches take
// it; semantics in include/longbow_gpu.h, lb_gpu_ivf_search): the tile that scores 128 rows of a list against up to 64 of the
// queries that probe it on the i8 matrix cores.  The grouping of a batch's pairs by list is the float32 tile's
// (kernels_ivf_group.hip: launch_ivf_group), and so are the work items and the walk; the tile's shape, its stage, its fragment
// reads and its transposed epilogue are the int8 tile's (kernels_ivf_i8_group.hip).
//
// Why.  ivf_scan_u8_kernel (kernels_ivf_u8.hip) stages a list once for every (query, probe slot) pair that probes it and scores
// it one lane a row.  Its value is a function of exact integers (lb_u8_exact.h): of the total S while S <= 2^24, of the four
// chain sums S_j over the residues i mod 4 while every S_j <= 2^24, and integer sums leave the same bits in any order, so
// v_mfma_i32_32x32x32_i8 may form them, 32 rows and 32 queries an instruction.
//
// Signed bytes.  The matrix cores multiply signed bytes, so every real row and query byte is shifted by 128 (^ 0x80808080) as it
// is staged; pieces at or beyond D stay zero.  (x - 128) - (q - 128) = x - q, so S = |x'|^2 + |q'|^2 - 2 x'.q' with no correction
// term, chain by chain as in total.  The norms are v_dot4_i32_i8 of the shifted pieces with themselves at staging, summed over a
// tile's chunks and then over the eight lanes that hold a row; nothing is stored beside the bytes.
//
// Two forms, a template argument as in the per-pair kernel:
//   totals (D <= 258)  no pair can exceed 2^24 (258 * 65025 < 2^24): the int8 tile's instruction stream, one accumulator a
//                      query column, JN in {1, 2} columns a workgroup, value u8_value_of_s(S).
//   chains (D > 258)   the four S_j are needed apart.  With D % 16 == 0 chain j is byte j of every 4-byte word, so a thread
//                      transposes the 4 x 4 bytes of its 16-byte piece in registers (eight v_perm_b32) and writes word
//                      t_j = (byte j of w0, w1, w2, w3) to row 144 + 32 j + 4 sp: a row's 128-byte chunk lies as [chain 0 | chain 1
//                      | chain 2 | chain 3], 32 bytes each, queries alike (equal k meet in A and B), and K-step j of the chunk
//                      accumulates x'_j.q'_j alone into acc[j].  The MFMA count is the int8 tile's; the accumulators are four
//                      times as many, so a workgroup takes ONE query column of 32 (64 accumulator registers): the column is the
//                      low bit of the item coordinate, a workgroup whose column is empty returns at once, and the sibling
//                      column finds the list's rows in L2.  A partial last chunk leaves zeros in every chain's K-step, so no
//                      K-step is skipped.  The epilogue is ivf_scan_u8_kernel<true>'s finish, bit for bit: u8_value_of_chains
//                      while max S_j <= 2^24, else (reachable for D > 1032 only) the lane evaluates that one pair's chain
//                      arithmetic from global memory, divergent on purpose.
//   Integer range, chains: a chain has D / 4 <= 2048 shifted bytes in [-128, 127]: |acc_j| <= 2048 * 2^14 = 2^25, the norms
//   likewise, nx_j + qn_j <= 2^26, 2 acc_j within +-2^26, and S_j = sum (x - q)^2 <= 2048 * 65025 < 2^28: all inside int32.
//   Totals: D <= 256, every quantity below 2^24.
//
// The ds_write_b32 of the chains form.  A wave's 64 lanes write word 36 sr + 8 j + sp for eight rows sr and eight pieces sp.
// 36 r mod 32 = 4 r: the second row's eight words overlap the first row's banks by four, and so on, so on 32 banks by half-waves
// (rows r .. r + 3) half of the banks are hit twice -- a two-way conflict on half of each store -- and on 64 banks only rows 0
// and 7 of a wave meet, on four banks.  A permutation of k inside a K-step has to be the same for every row and query (every row
// meets every query), so it cannot remove that; a cross-lane 4 x 4 word transpose into ds_write_b128 costs more vector
// instructions than the conflict costs LDS cycles.  Left as it is, unmeasured: a thread's stage is 20 such stores (80 B) beside
// 8 ds_read_b128 (128 B), so they are no small part of the LDS traffic.
// No FMA contraction here.
#include "lb_device.h"
#include "lb_ivf_u8.h"
#include "lb_list_scan.h"
#include "lb_u8_exact.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int U8G_THREADS = 256;
constexpr int U8G_ROWS = 128;                       // rows per tile: 32 a wave
constexpr int U8G_COL = 32;                         // queries per column
constexpr int U8G_CK = 128;                         // bytes per row and query per stage: four K-steps of 32
constexpr int U8G_LD = U8G_CK + 16;                 // LDS row stride (bytes)
constexpr int U8G_PPR = U8G_CK / 16;                // 16-byte pieces per row per stage == lanes that share a row
constexpr int U8G_XPT = U8G_ROWS * U8G_PPR / U8G_THREADS; // row pieces per thread per stage (4); a query column is one each
constexpr int U8G_STAGE = (U8G_ROWS + IVF_GROUP_PAIRS) * U8G_LD; // 27,648 B
constexpr int U8G_TLD = U8G_ROWS + 1;               // floats per query of the transposed distances
constexpr int U8G_SHIFT = (int)0x80808080u;         // uint8 -> the signed byte 128 below it, four at a time
static_assert(U8G_COL * U8G_PPR == U8G_THREADS && U8G_XPT * U8G_COL == U8G_ROWS, "a thread stages piece tid % 8 of row and query tid / 8 + 32 i");
static_assert(U8G_COL * U8G_TLD * 4 <= U8G_STAGE, "one query column's distances fit the free stage");

// What a workgroup's item is, wave-uniform
struct U8GroupWork {
    uint32_t len;          // rows of the list
    const uint32_t *rmap;  // the list's rows, ascending
    const uint32_t *pairs; // the group's pairs
    int gn;                // pairs of the group, 1 .. 64
    int col0;              // the first query column of this workgroup (chains form: its only one)
};

// the sum over the eight consecutive lanes that hold one row's pieces, in all of them
__device__ __forceinline__ int u8g_sum8(int v)
{
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v + __shfl_xor(v, 4);
}

// (w0, w1, w2, w3) -> (t0, t1, t2, t3), t_j = byte j of w0 | byte j of w1 << 8 | byte j of w2 << 16 | byte j of w3 << 24.
// v_perm_b32 d, s0, s1, sel: selector bytes 0..3 pick the bytes of s1, 4..7 those of s0
__device__ __forceinline__ i32x4 u8g_transpose(const i32x4 w)
{
    const uint32_t lo01 = __builtin_amdgcn_perm((uint32_t)w.y, (uint32_t)w.x, 0x05010400u); // w0.b0 w1.b0 w0.b1 w1.b1
    const uint32_t hi01 = __builtin_amdgcn_perm((uint32_t)w.y, (uint32_t)w.x, 0x07030602u); // w0.b2 w1.b2 w0.b3 w1.b3
    const uint32_t lo23 = __builtin_amdgcn_perm((uint32_t)w.w, (uint32_t)w.z, 0x05010400u);
    const uint32_t hi23 = __builtin_amdgcn_perm((uint32_t)w.w, (uint32_t)w.z, 0x07030602u);
    return i32x4{(int)__builtin_amdgcn_perm(lo23, lo01, 0x05040100u), (int)__builtin_amdgcn_perm(lo23, lo01, 0x07060302u),
                 (int)__builtin_amdgcn_perm(hi23, hi01, 0x05040100u), (int)__builtin_amdgcn_perm(hi23, hi01, 0x07060302u)};
}

// One held piece into the stage at `dst` (its row's or query's chunk), shifted if it is real, and its share of the norms into
// n[0 .. NA): per chain, or all of it in n[0].  reset: the tile's (the group's) first chunk
template <bool CHAINS>
__device__ __forceinline__ void u8g_put(int8_t *dst, int sp, i32x4 v, bool real, bool reset, int (&n)[CHAINS ? 4 : 1])
{
    if (real) v ^= i32x4{U8G_SHIFT, U8G_SHIFT, U8G_SHIFT, U8G_SHIFT};
    if (CHAINS) {
        v = u8g_transpose(v);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            *reinterpret_cast<int *>(&dst[32 * j + 4 * sp]) = v[j];
            n[j] = __builtin_amdgcn_sdot4(v[j], v[j], reset ? 0 : n[j], false);
        }
    } else {
        *reinterpret_cast<i32x4 *>(&dst[16 * sp]) = v;
        int t = reset ? 0 : n[0];
#pragma unroll
        for (int j = 0; j < 4; j++) t = __builtin_amdgcn_sdot4(v[j], v[j], t, false);
        n[0] = t;
    }
}

// JN: query columns of 32 this workgroup scores, from column w.col0 (chains form: 1).  NA accumulators and norms a pair: the four
// chains, or the total.  lnx[r NA + j]: |x'_j|^2 of row r of the tile; lqn[c NA + j]: |q'_j|^2 of the group's c-th pair's query;
// s_base[c]: where the keys of that pair start, -1 for a pair whose keys would leave its query's pmax.
template <bool CHAINS, int JN>
__device__ __forceinline__ void ivf_u8_tile_body(const IvfU8Scan &s, const U8GroupWork &w, int8_t *lds, int *lnx, int *lqn, const int64_t *s_base)
{
    constexpr int NA = CHAINS ? 4 : 1;
    static_assert(!CHAINS || JN == 1, "the chains form takes one column a workgroup");
    const IvfBatch &a = s.b;
    int8_t *lx = lds, *lq = lds + U8G_ROWS * U8G_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sp = tid & (U8G_PPR - 1), sr = tid / U8G_PPR; // staging: piece sp of row sr + 32 i of the tile, of query sr + 32 j of the group
    const int D = a.D;
    const int nchunks = (D + U8G_CK - 1) / U8G_CK;
    const uint32_t ntiles = (w.len + U8G_ROWS - 1) / U8G_ROWS;
    const int q0 = w.col0 * U8G_COL; // the first pair of the group this workgroup scores

    i32x4 px[U8G_XPT], pq[JN];
    uint32_t xrow[U8G_XPT], qoff[JN]; // (a batch's queries hold fewer than 2^31 bytes)
    int nxp[U8G_XPT][NA], nqp[JN][NA]; // this thread's share of the norms of its rows of the tile, of its queries
#pragma unroll
    for (int j = 0; j < JN; j++) qoff[j] = w.pairs[std::min(q0 + sr + U8G_COL * j, w.gn - 1)] / (uint32_t)a.np * (uint32_t)D;
    auto load_stage = [&](uint32_t tile, int c) {
        const int k = c * U8G_CK + sp * 16;
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < U8G_XPT; i++) {
                uint32_t pos = tile * U8G_ROWS + sr + U8G_COL * i;
                if (pos >= w.len) pos = w.len - 1; // (computed, never written)
                xrow[i] = w.rmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < U8G_XPT; i++) {
            px[i] = i32x4{0, 0, 0, 0};
            // (a plain load: other groups and the sibling column of the same list find the rows in L2 / MALL)
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
        const bool real = c * U8G_CK + sp * 16 < D;
#pragma unroll
        for (int i = 0; i < U8G_XPT; i++) u8g_put<CHAINS>(&lx[(sr + U8G_COL * i) * U8G_LD], sp, px[i], real, c == 0, nxp[i]);
#pragma unroll
        for (int j = 0; j < JN; j++) {
            int unused[NA] = {}; // (the queries' norms stay from the first tile)
            if (first) u8g_put<CHAINS>(&lq[(sr + U8G_COL * j) * U8G_LD], sp, pq[j], real, c == 0, nqp[j]);
            else u8g_put<CHAINS>(&lq[(sr + U8G_COL * j) * U8G_LD], sp, pq[j], real, true, unused);
        }
        if (c != nchunks - 1) return;
#pragma unroll
        for (int i = 0; i < U8G_XPT; i++)
#pragma unroll
            for (int h = 0; h < NA; h++) {
                const int t = u8g_sum8(nxp[i][h]);
                if (sp == 0) lnx[(sr + U8G_COL * i) * NA + h] = t;
            }
        if (first) {
#pragma unroll
            for (int j = 0; j < JN; j++)
#pragma unroll
                for (int h = 0; h < NA; h++) {
                    const int t = u8g_sum8(nqp[j][h]);
                    if (sp == 0) lqn[(sr + U8G_COL * j) * NA + h] = t;
                }
        }
    };

    // totals [column j][0]: x'.q' of row 32 wave + (e & 3) + 8 (e >> 2) + 4 (lane >> 5) and the column's query lane & 31;
    // chains [0][chain h]: x'_h.q'_h of that row and query
    i32x16 acc[JN][NA];
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
                for (int h = 0; h < NA; h++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[j][h][e] = 0;
        }
        // totals: K-steps that are all padding are not issued; chains: every K-step is a chain
        const int ksteps = CHAINS ? U8G_CK / 32 : (std::min(D - c * U8G_CK, U8G_CK) + 31) >> 5;
#pragma unroll
        for (int st = 0; st < U8G_CK / 32; st++) {
            if (st >= ksteps) break; // (uniform)
            const int off = st * 32 + (lane >> 5) * 16;
            const i32x4 fa = *reinterpret_cast<const i32x4 *>(&lx[(wave * 32 + (lane & 31)) * U8G_LD + off]);
#pragma unroll
            for (int j = 0; j < JN; j++) {
                const i32x4 fb = *reinterpret_cast<const i32x4 *>(&lq[(j * U8G_COL + (lane & 31)) * U8G_LD + off]);
                i32x16 &d = acc[j][CHAINS ? st : 0];
                d = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, d, 0, 0, 0);
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (c == nchunks - 1) {
            // a column's distances through the free stage, [query][row]; then a wave a query, a lane a list position
            float *lt = reinterpret_cast<float *>(lds);
            const uint32_t pos0 = tile * U8G_ROWS + lane, pos1 = pos0 + 64;
            const uint32_t row0 = pos0 < w.len ? w.rmap[pos0] : 0u, row1 = pos1 < w.len ? w.rmap[pos1] : 0u;
#pragma unroll
            for (int j = 0; j < JN; j++) {
                const int cq = j * U8G_COL + (lane & 31); // this lane's query, of the workgroup's
                const int rl0 = wave * 32 + 4 * (lane >> 5);
                int qn[NA];
#pragma unroll
                for (int h = 0; h < NA; h++) qn[h] = lqn[cq * NA + h];
                uint32_t beyond = 0; // chains: bit e, a pair with a chain past 2^24
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int rl = rl0 + (e & 3) + 8 * (e >> 2);
                    float dist = 0.f;
                    if (!CHAINS) { // 0 <= S <= 256 * 65025 < 2^24
                        dist = u8_value_of_s((uint32_t)(lnx[rl] + qn[0] - 2 * acc[j][0][e]));
                    } else { // 0 <= S_h < 2^28 (the bounds above)
                        uint32_t S[4];
#pragma unroll
                        for (int h = 0; h < 4; h++) S[h] = (uint32_t)(lnx[rl * NA + h] + qn[h] - 2 * acc[j][h][e]);
                        if (std::max(std::max(S[0], S[1]), std::max(S[2], S[3])) <= U8_EXACT_S) dist = u8_value_of_chains(S[0], S[1], S[2], S[3]);
                        else beyond |= 1u << e;
                    }
                    lt[(lane & 31) * U8G_TLD + rl] = dist;
                    __builtin_amdgcn_sched_barrier(0); // (one row's norms in flight, not sixteen)
                }
                // only for D > 1032: such a pair is evaluated as the reference writes it, from global memory (what is never
                // written is not evaluated: a row past the list's end, a query past the group's)
                if (CHAINS && q0 + cq < w.gn) {
                    const uint8_t *qv = s.Q + (int64_t)(w.pairs[q0 + cq] / (uint32_t)a.np) * D;
                    while (beyond) {
                        const int e = __builtin_ctz(beyond);
                        beyond &= beyond - 1;
                        const int rl = rl0 + (e & 3) + 8 * (e >> 2);
                        const uint32_t pos = tile * U8G_ROWS + rl;
                        if (pos < w.len) lt[(lane & 31) * U8G_TLD + rl] = (float)sqrt((double)u8_chain_sum<true>(s.X + (int64_t)w.rmap[pos] * D, qv, D));
                    }
                }
                __syncthreads();
                const int nj = std::min(w.gn - q0 - j * U8G_COL, U8G_COL);
                for (int jq = wave; jq < nj; jq += U8G_THREADS / 64) {
                    const int64_t base = s_base[q0 + j * U8G_COL + jq];
                    if (base < 0) continue;
                    if (pos0 < w.len) a.keys[base + pos0] = pack_entry(lt[jq * U8G_TLD + lane], row0);
                    if (pos1 < w.len) a.keys[base + pos1] = pack_entry(lt[jq * U8G_TLD + lane + 64], row1);
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

// ivf_scan_u8_staged holds; CHAINS false: D <= 258.  The item coordinate is blockIdx.y + blockIdx.z gridDim.y: the item itself in
// the totals form, (item, query column) in the chains form.  LDS: the stage (27,648 B), the tile's row norms (512 B, chains
// 2,048), the group's query norms (256 B, chains 1,024) and key bases (512 B).
template <bool CHAINS>
__global__ __launch_bounds__(U8G_THREADS, CHAINS ? 3 : 4) void ivf_scan_u8_tile_kernel(IvfU8Scan s, IvfGroups g)
{
    constexpr int NA = CHAINS ? 4 : 1;
    __shared__ __attribute__((aligned(16))) int8_t lds[U8G_STAGE];
    __shared__ int lnx[U8G_ROWS * NA];
    __shared__ int lqn[IVF_GROUP_PAIRS * NA];
    __shared__ int64_t s_base[IVF_GROUP_PAIRS];
    const IvfBatch &a = s.b;
    const uint32_t coord = blockIdx.y + blockIdx.z * gridDim.y;
    const uint32_t item = CHAINS ? coord >> 1 : coord;
    if (item >= g.nitems[0]) return;
    const uint2 it = g.items[item]; // (list, first pair): the list is below nlist and has rows
    const uint32_t off = a.L.off[it.x];
    U8GroupWork w;
    w.len = a.L.off[it.x + 1] - off;
    if ((uint64_t)blockIdx.x * U8G_ROWS >= w.len) return;
    w.rmap = a.L.rows + off;
    w.pairs = g.gpairs + it.y;
    w.gn = (int)std::min<uint32_t>(g.goff[it.x + 1] - it.y, IVF_GROUP_PAIRS);
    w.col0 = CHAINS ? (int)(coord & 1) : 0;
    if (w.col0 * U8G_COL >= w.gn) return; // (chains: the group has no second column)
    if ((int)threadIdx.x < w.gn) {
        const uint32_t pair = w.pairs[threadIdx.x];
        const uint32_t q = pair / (uint32_t)a.np, p = pair % (uint32_t)a.np;
        const uint32_t seg = a.seg[(int64_t)q * (a.np + 1) + p];
        // never refused with distinct probes: the keys of a query stay inside its pmax
        s_base[threadIdx.x] = (int64_t)seg + w.len > a.pmax ? -1 : (int64_t)q * a.pmax + seg;
    }
    // (the body's first barrier comes before any read of s_base)
    if (CHAINS || w.gn <= U8G_COL) ivf_u8_tile_body<CHAINS, 1>(s, w, lds, lnx, lqn, s_base); // uniform: an empty query column costs nothing
    else ivf_u8_tile_body<CHAINS, CHAINS ? 1 : 2>(s, w, lds, lnx, lqn, s_base);
}

hipError_t launch_ivf_scan_u8_tile(const IvfU8Scan &a, const IvfGroups &g, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.b.nq * a.b.np;
    if (pairs <= 0 || maxlen <= 0) return hipSuccess;
    const hipError_t e = launch_ivf_group(a.b, g, s);
    if (e != hipSuccess) return e;
    const bool chains = a.b.D > IVF_U8_TOTALS_D;
    const int64_t items = ivf_group_max_items(pairs, a.b.L.nlist), tiles = (maxlen + U8G_ROWS - 1) / U8G_ROWS;
    const int64_t coords = chains ? 2 * items : items; // <= 2 (1024 * 65536 / 64 + 65536) = 2^21 + 2^17: z stays below 65536
    const unsigned gy = (unsigned)std::min<int64_t>(coords, IVF_PAIRS_Y);
    const dim3 grid((unsigned)list_scan_gx(items, tiles), gy, (unsigned)((coords + gy - 1) / gy));
    if (chains) hipLaunchKernelGGL((ivf_scan_u8_tile_kernel<true>), grid, dim3(U8G_THREADS), 0, s, a, g);
    else hipLaunchKernelGGL((ivf_scan_u8_tile_kernel<false>), grid, dim3(U8G_THREADS), 0, s, a, g);
    return hipSuccess;
}

} // namespace lb
