// kernels_ivf_group.hip -- the list-major form of the IVF-Flat list scan over float32 rows (ivf.hip decides which batches take it;
// semantics in include/longbow_gpu.h, lb_gpu_ivf_search): the grouping of a batch's (query, probe slot) pairs by the list they
// probe, and the tile that scores 64 rows of a list against up to 64 of the queries that probe it.
//
// Why.  ivf_scan_kernel (kernels_ivf.hip) stages a list once for every pair that probes it; a batch whose queries share lists
// moves every row through L2 and LDS as many times as it has queries there.  Here a staged element of a row meets up to 64
// queries, and a staged element of a query 64 rows.
//
// The grouping.  The pairs are sorted by list with the handle's own stable counting sort (launch_ivf_sort: a pair is a "row",
// its list the bucket; a probe outside [0, nlist) gets a bucket the sort drops), which leaves list l's pairs as the run
// gpairs[goff[l], goff[l + 1]) in ascending pair order.  One workgroup then cuts every run of a non-empty list into groups of at
// most 64 pairs: the work items (list, first pair of the group), and their number, which stays on the device.  The host sizes
// the grid by ceil(pairs / 64) + min(nlist, pairs), which no such cut exceeds; workgroups past the count leave at once.
//
// The tile (ivt_estep_kernel's, kernels_ivf_train.hip, with queries where it has centroids).  A 256-thread workgroup takes one
// item and walks the list's 64-row tiles blockIdx.x, blockIdx.x + gridDim.x, ..., a tile in chunks of 64 elements: one LDS
// stage [64 row chunks | 64 query chunks] at the padded stride IG_LD, the next stage's global loads held in registers
// meanwhile, wrapping from a tile's last chunk to the next tile's first (ivf_scan_kernel's pipeline).  Lane (ty, tx) = (tid / 16,
// tid % 16) keeps the 4 x JN pairs of rows ty + 16 i and queries tx + 16 j, each pair an Acc<ORDER>, and under cosine one
// ||x||^2 accumulator per row.  Every group of four elements enters every chain as in ivf_scan_kernel and the finish is the
// same exact_distance, so a key equals that kernel's key bit for bit.  JN = ceil(group size / 16) is uniform over the
// workgroup and a template argument of the body: a group of 17 pairs pays for two query columns, not four, in loads, LDS
// traffic and arithmetic alike.  The query operands go through LDS and not through scalar loads: a lane's four queries differ
// from its neighbour's (tx), which is what lets 16 lanes share one row read, and 64 x 64 floats a chunk do not fit the SGPR file.
//
// The keys.  After a tile's last chunk the stage is free: the 64 x 64 distances are transposed through it ([query][row], stride
// IG_LD, conflict-free both ways), and wave w then writes queries w, w + 4, ... of the group, lane = position in the tile, so
// that a wave's stores for one query are 512 consecutive bytes of keys[q pmax + seg[q][p] + pos].
// No FMA contraction here.
#include "lb_device.h"
#include "lb_exact.h"
#include "lb_ivf.h"
#include "lb_list_scan.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

constexpr int IG_THREADS = 256;
constexpr int IG_ROWS = 64;       // rows per tile
constexpr int IG_DK = 64;         // floats per row per stage
constexpr int IG_LD = IG_DK + 4;  // padded LDS row stride (floats): IT_LD / IV_LD's, conflict-free ds_read_b128
constexpr int IG_PER = 4;         // rows per lane; query columns per lane at most
constexpr uint32_t IG_NO_LIST = 0xffffffffu;

// ---- the grouping -----------------------------------------------------------------------------------------------------------
// bucket[pair] = the list the pair probes, or a bucket that launch_ivf_sort drops
__global__ void ivf_group_bucket_kernel(const int64_t *probes, int64_t pairs, int nlist, uint32_t *bucket)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = probes[i];
        bucket[i] = l >= 0 && l < nlist ? (uint32_t)l : IG_NO_LIST;
    }
}

// One workgroup; thread t takes the lists [t per, t per + per).  A list with rows and c pairs gives ceil(c / 64) items, in list
// order: item = (list, first pair of the group in gpairs).  nitems[0] = their number (at most max_items, the host's bound).
__global__ __launch_bounds__(1024) void ivf_group_items_kernel(IvfGroups g, IvfLists L)
{
    __shared__ uint32_t s_scan[1024];
    const int t = threadIdx.x;
    const int per = (L.nlist + 1023) / 1024;
    const int b = std::min(t * per, L.nlist), e = std::min(b + per, L.nlist);
    auto groups_of = [&](int l) -> uint32_t {
        if (L.off[l + 1] == L.off[l]) return 0u; // an empty list: its pairs have nothing to scan
        return (g.goff[l + 1] - g.goff[l] + IVF_GROUP_PAIRS - 1) / IVF_GROUP_PAIRS;
    };
    uint32_t sum = 0;
    for (int l = b; l < e; l++) sum += groups_of(l);
    s_scan[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t add = t >= o ? s_scan[t - o] : 0u;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    uint32_t at = s_scan[t] - sum;
    for (int l = b; l < e; l++) {
        const uint32_t n = groups_of(l), first = g.goff[l];
        for (uint32_t i = 0; i < n; i++, at++)
            if (at < g.max_items) g.items[at] = make_uint2((uint32_t)l, first + i * IVF_GROUP_PAIRS);
    }
    if (t == 1023) g.nitems[0] = std::min(s_scan[1023], g.max_items);
}

// ---- the tile ---------------------------------------------------------------------------------------------------------------
// What a workgroup's item is, wave-uniform
struct GroupWork {
    uint32_t len;         // rows of the list
    const uint32_t *rmap; // the list's rows, ascending
    const uint32_t *pairs; // the group's pairs
    int gn;               // pairs of the group, 1 .. 64
};

// JN: query columns of 16 that hold a pair of the group.  s_base[j]: where the keys of the group's j-th pair start, -1 for a
// pair whose keys would leave its query's pmax (ivf_list_work's guard).
template <int METRIC, int ORDER, int JN>
__device__ __forceinline__ void ivf_tile_body(const IvfBatch &a, const GroupWork &w, float *lds, const int64_t *s_base)
{
    float *lx = lds, *lq = lds + IG_ROWS * IG_LD;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wave = tid >> 6;
    const int D = a.D;
    const int nchunks = (D + IG_DK - 1) / IG_DK;
    const uint32_t ntiles = (w.len + IG_ROWS - 1) / IG_ROWS;

    // staging slot i of this lane: piece tx of row ty + 16 i of the tile, and of query ty + 16 i of the group (i < JN)
    f32x4 sx[IG_PER], sq[JN];
    uint32_t xrow[IG_PER], qoff[JN]; // (a batch's queries hold fewer than 2^31 floats)
    float na[JN]; // ||q||^2 of the queries this lane scores: tx + 16 j
#pragma unroll
    for (int j = 0; j < JN; j++) {
        qoff[j] = w.pairs[std::min(ty + 16 * j, w.gn - 1)] / (uint32_t)a.np * (uint32_t)D;
        na[j] = METRIC == METRIC_COS ? a.qna[w.pairs[std::min(tx + 16 * j, w.gn - 1)] / (uint32_t)a.np] : 0.f;
    }
    auto load_stage = [&](uint32_t tile, int c) {
        int k = c * IG_DK + tx * 4;
        if (k > D - 4) k = D - 4; // (a piece past D is never consumed)
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < IG_PER; i++) {
                uint32_t pos = tile * IG_ROWS + ty + 16 * i;
                if (pos >= w.len) pos = w.len - 1; // (computed, never written)
                xrow[i] = w.rmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < IG_PER; i++) sx[i] = *reinterpret_cast<const f32x4 *>(a.X + (int64_t)xrow[i] * D + k);
#pragma unroll
        for (int j = 0; j < JN; j++) sq[j] = *reinterpret_cast<const f32x4 *>(a.Q + qoff[j] + k);
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < IG_PER; i++) *reinterpret_cast<f32x4 *>(&lx[(ty + 16 * i) * IG_LD + tx * 4]) = sx[i];
#pragma unroll
        for (int j = 0; j < JN; j++) *reinterpret_cast<f32x4 *>(&lq[(ty + 16 * j) * IG_LD + tx * 4]) = sq[j];
    };

    Acc<ORDER> acc[IG_PER][JN]; // [row ty + 16 i][query tx + 16 j]: L2 sum (q-x)^2 ; cos/dot sum q*x
    Acc<ORDER> nb[IG_PER];      // cos: sum x*x of row ty + 16 i

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
            for (int i = 0; i < IG_PER; i++) {
                nb[i].zero();
#pragma unroll
                for (int j = 0; j < JN; j++) acc[i][j].zero();
            }
        }
        const int d0 = c * IG_DK;
        const int nfull4 = (min(D, d0 + IG_DK) - d0) >> 2;
#pragma unroll 2
        for (int g = 0; g < nfull4; g++) {
            f32x4 xv[IG_PER], qv[JN];
#pragma unroll
            for (int i = 0; i < IG_PER; i++) xv[i] = *reinterpret_cast<const f32x4 *>(&lx[(ty + 16 * i) * IG_LD + g * 4]);
#pragma unroll
            for (int j = 0; j < JN; j++) qv[j] = *reinterpret_cast<const f32x4 *>(&lq[(tx + 16 * j) * IG_LD + g * 4]);
#pragma unroll
            for (int i = 0; i < IG_PER; i++) {
                if (METRIC == METRIC_COS) nb[i].add4_sq(xv[i]);
#pragma unroll
                for (int j = 0; j < JN; j++) acc[i][j].template add4_pair<METRIC>(qv[j], xv[i]);
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (c == nchunks - 1) {
            // the tile's distances through the free stage, [query][row]; then a wave a query, a lane a list position
            float *lt = lds;
#pragma unroll
            for (int i = 0; i < IG_PER; i++) {
                const float nbt = nb[i].total();
#pragma unroll
                for (int j = 0; j < JN; j++)
                    lt[(tx + 16 * j) * IG_LD + ty + 16 * i] = exact_distance<METRIC>(acc[i][j].total(), nbt, na[j], D, false);
            }
            __syncthreads();
            const uint32_t pos = tile * IG_ROWS + lane;
            if (pos < w.len) {
                const uint32_t row = w.rmap[pos];
                for (int j = wave; j < w.gn; j += IG_THREADS / 64) {
                    const int64_t base = s_base[j];
                    if (base >= 0) a.keys[base + pos] = pack_entry(lt[j * IG_LD + lane], row);
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

// D % 4 == 0, X and Q 16-byte aligned.  LDS: the stage (34,816 B) and the group's key bases (512 B).
template <int METRIC, int ORDER>
__global__ __launch_bounds__(IG_THREADS, 2) void ivf_scan_tile_kernel(IvfBatch a, IvfGroups g)
{
    __shared__ __attribute__((aligned(16))) float lds[2 * IG_ROWS * IG_LD];
    __shared__ int64_t s_base[IVF_GROUP_PAIRS];
    const uint32_t item = blockIdx.y + blockIdx.z * gridDim.y;
    if (item >= g.nitems[0]) return;
    const uint2 it = g.items[item]; // (list, first pair): the list is below nlist and has rows
    const uint32_t off = a.L.off[it.x];
    GroupWork w;
    w.len = a.L.off[it.x + 1] - off;
    if ((uint64_t)blockIdx.x * IG_ROWS >= w.len) return;
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
    switch ((w.gn + 15) >> 4) { // uniform over the workgroup: whole empty query columns cost nothing
    case 1: ivf_tile_body<METRIC, ORDER, 1>(a, w, lds, s_base); break;
    case 2: ivf_tile_body<METRIC, ORDER, 2>(a, w, lds, s_base); break;
    case 3: ivf_tile_body<METRIC, ORDER, 3>(a, w, lds, s_base); break;
    default: ivf_tile_body<METRIC, ORDER, 4>(a, w, lds, s_base); break;
    }
}

hipError_t launch_ivf_group(const IvfBatch &a, const IvfGroups &g, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.nq * a.np;
    hipLaunchKernelGGL(ivf_group_bucket_kernel, dim3((unsigned)std::min<int64_t>((pairs + 255) / 256, 4096)), dim3(256), 0, s, a.probes, pairs,
                       a.L.nlist, g.bucket);
    const hipError_t e = launch_ivf_sort(g.bucket, pairs, a.L.nlist, g.hist, g.goff, g.gpairs, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ivf_group_items_kernel, dim3(1), dim3(1024), 0, s, g, a.L);
    return hipSuccess;
}

hipError_t launch_ivf_scan_tile(int metric, int order, const IvfBatch &a, const IvfGroups &g, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.nq * a.np;
    if (pairs <= 0 || maxlen <= 0) return hipSuccess;
    const hipError_t e = launch_ivf_group(a, g, s);
    if (e != hipSuccess) return e;
    const int64_t items = ivf_group_max_items(pairs, a.L.nlist), tiles = (maxlen + IG_ROWS - 1) / IG_ROWS;
    const unsigned gy = (unsigned)std::min<int64_t>(items, IVF_PAIRS_Y);
    const dim3 grid((unsigned)list_scan_gx(items, tiles), gy, (unsigned)((items + gy - 1) / gy));
    with_metric_order(metric, order, [&](auto m, auto o) {
        hipLaunchKernelGGL((ivf_scan_tile_kernel<decltype(m)::value, decltype(o)::value>), grid, dim3(IG_THREADS), 0, s, a, g);
    });
    return hipSuccess;
}

} // namespace lb
