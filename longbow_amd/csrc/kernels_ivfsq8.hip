// kernels_ivfsq8.hip -- the IVF-SQ8 index (ivfsq8.hip; semantics in include/longbow_gpu.h, lb_gpu_ivfsq8_*): the scan of the
// probed lists over uint8 rows and the selection of the k smallest of a query's integer keys.  The plan of a batch, the lists and
// the visible lists are kernels_ivf.hip's, the codec and the norms kernels_sq8.hip's.
//
// The codes stay in insertion order at a stride of dims rounded up to 16 bytes, pad bytes zero, and a list is an ascending array
// of row numbers, so the list scan is the list scans' walk (lb_list_scan.h) over the tile body of sq8_dist_kernel<QT, true>
// (kernels_sq8.hip): a list per (query, probe slot), one lane per row, the rows' bytes gathered by row number in coalesced
// 16-byte pieces into an LDS tile whose row stride is an odd number of 16-byte slots, the query's code in LDS and read
// wave-uniform.  x.q and |x|^2 both come from v_dot4_u32_u8 on the piece a lane holds, and S = |x|^2 + |q|^2 - 2 x.q in
// integers: at most 65025 * 8192 < 2^30, nothing wraps.  Every scanned row leaves one key (S << 32) | row: S < 2^31, so the
// u64 order of the keys is the (S, row) order of the integers and kEntryMax padding sorts last.  Integer only.
#include "lb_device.h"
#include "lb_ivfsq8.h"
#include "lb_list_scan.h"
#include "lb_select.h"

#include <float.h>
#include <algorithm>

namespace lb {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int ISQ_CH = 8;                // 16-byte pieces of a row per stage: one 128-byte line of the row
constexpr int ISQ_LD = ISQ_CH + 1;       // LDS row stride in pieces: odd, so the 16 lanes of a ds_read_b128 group fall on 16 slots

__device__ __forceinline__ uint32_t isq_dot16(const u32x4 a, const u32x4 b, uint32_t acc)
{
    acc = __builtin_amdgcn_udot4(a.x, b.x, acc, false);
    acc = __builtin_amdgcn_udot4(a.y, b.y, acc, false);
    acc = __builtin_amdgcn_udot4(a.z, b.z, acc, false);
    acc = __builtin_amdgcn_udot4(a.w, b.w, acc, false);
    return acc;
}

} // namespace

// Work = (query, probe slot, 128-row tile of that list), found as lb_list_scan.h states and walked as it states, in this
// kernel's own text (below).  A stage is 128 rows x 8 pieces, with a register-held prefetch of the next one; the query's whole
// code lies behind the stage, zero past its last piece.
// LDS: tile u32x4[ISQ_ROWS][ISQ_LD] | query u32x4[nchunks * ISQ_CH]
__global__ __launch_bounds__(ISQ_ROWS) void ivfsq8_scan_kernel(IvfSq8Scan a)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 isq_smem[];
    u32x4 *lrow = isq_smem;
    u32x4 *lq = lrow + ISQ_ROWS * ISQ_LD;
    ListWork w;
    if (!ivf_list_work(a.b, ISQ_ROWS, w)) return;
    const int tid = threadIdx.x;
    const int P = a.stride >> 4, nchunks = (P + ISQ_CH - 1) / ISQ_CH;
    const uint32_t ntiles = (w.len + ISQ_ROWS - 1) / ISQ_ROWS;
    const u32x4 *codes = reinterpret_cast<const u32x4 *>(a.codes);
    const u32x4 *q_src = reinterpret_cast<const u32x4 *>(a.qcodes) + (int64_t)w.q * P;
    const uint32_t qn = (uint32_t)a.qnorms[w.q];
    const uint32_t last_row = (uint32_t)(a.n - 1);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int idx = tid; idx < nchunks * ISQ_CH; idx += ISQ_ROWS) lq[idx] = idx < P ? q_src[idx] : zero;

    // a thread's ISQ_CH staging slots of a stage: piece tid % 8 of the rows tid / 8 + 16 i of the tile
    u32x4 stg[ISQ_CH];
    uint32_t rid[ISQ_CH]; // the rows behind them, of the tile being loaded
    const int pv = tid & (ISQ_CH - 1);
    auto load_stage = [&](uint32_t tile, int c) {
        const uint32_t trow0 = tile * ISQ_ROWS;
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < ISQ_CH; i++) {
                uint32_t pos = trow0 + ((uint32_t)(tid + ISQ_ROWS * i) >> 3);
                if (pos >= w.len) pos = w.len - 1;
                const uint32_t r = w.rmap[pos];
                rid[i] = r < last_row ? r : last_row;
            }
        }
        int p = c * ISQ_CH + pv;
        if (p > P - 1) p = P - 1; // pieces past P are never consumed
#pragma unroll
        for (int i = 0; i < ISQ_CH; i++) {
            // (a plain load: other queries of the batch probe the same list and find it in L2 / MALL)
            stg[i] = codes[(int64_t)rid[i] * P + p];
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < ISQ_CH; i++) lrow[((tid + ISQ_ROWS * i) >> 3) * ISQ_LD + pv] = stg[i];
    };

    uint32_t dot = 0u, nn = 0u; // x.q and |x|^2 of this lane's row
    // a finished tile's key is written right after the next stage's loads are issued
    uint32_t pend_s = 0u, pend_tile = 0u;
    bool pending = false;
    auto flush = [&]() {
        const uint32_t pos = pend_tile * ISQ_ROWS + tid;
        if (pos < w.len) w.out[pos] = ((uint64_t)pend_s << 32) | (uint64_t)w.rmap[pos];
        pending = false;
    };

    // walk_list_tiles' walk (lb_list_scan.h) in this kernel's own text, kept in step with it by hand.  Built over the shared
    // walk the kernel came out nine instructions longer (same registers and occupancy) and its scan slot at 1024 queries x 32
    // probes 0.5 % slower in all three runs, four times the parent's spread (LABNOTES R34.1).
    uint32_t tile = blockIdx.x;
    int c = 0;
    load_stage(tile, 0);
    write_stage();
    __syncthreads(); // (the query's code too)
    while (true) {
        uint32_t ntile = tile;
        int nc = c + 1;
        if (nc == nchunks) {
            nc = 0;
            ntile = tile + gridDim.x;
        }
        const bool has_next = ntile < ntiles;
        if (has_next) load_stage(ntile, nc);
        if (pending) flush();
        if (c == 0) dot = nn = 0u;
        {
            const u32x4 *xr = lrow + tid * ISQ_LD;
            const u32x4 *qc = lq + c * ISQ_CH;
            const int nfull = min(P - c * ISQ_CH, ISQ_CH);
#pragma unroll
            for (int g = 0; g < ISQ_CH; g++) {
                if (g < nfull) { // (wave-uniform)
                    const u32x4 xv = xr[g];
                    dot = isq_dot16(xv, qc[g], dot);
                    nn = isq_dot16(xv, xv, nn);
                }
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (has_next) write_stage();
        if (c == nchunks - 1) {
            pend_s = nn + qn - 2u * dot;
            pend_tile = tile;
            pending = true;
        }
        __syncthreads();
        if (!has_next) break;
        tile = ntile;
        c = nc;
    }
    if (pending) flush();
}

void launch_ivfsq8_scan(const IvfSq8Scan &a, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.b.nq * a.b.np;
    if (pairs <= 0 || maxlen <= 0 || a.n <= 0) return;
    const int P = a.stride >> 4, Pq = (P + ISQ_CH - 1) / ISQ_CH * ISQ_CH;
    const size_t lds = ((size_t)ISQ_ROWS * ISQ_LD + (size_t)Pq) * 16; // at most 26,752 B (dims 8192)
    hipLaunchKernelGGL(ivfsq8_scan_kernel, ivf_scan_grid(pairs, maxlen, ISQ_ROWS), dim3(ISQ_ROWS), lds, s, a);
}

// ---- select ---------------------------------------------------------------------------------------------------------------
// One workgroup per query: the k smallest of its n = P_q unique u64 keys, ascending, with ivf_select_kernel's structure
// (kernels_ivf.hip) over lb_select.h's shared pieces:
//   n <= cap (the LDS copy's room): the keys are copied to LDS; with next_pow2(n) <= 2 Pk a bitonic sort of everything,
//   otherwise, and for every n > cap: radix_kth of the k-th smallest key (the counting passes read the LDS copy, or the keys in
//   global memory when they do not fit), compact_le of the k keys at or below it into LDS, a sort of those.
// The emit is this kernel's own: a key's upper half is S itself, reported as float32(S).
// LDS: keys u64[cap] | stage u64[Pk] | SelectScratch
constexpr int ISS_THREADS = 1024;

__global__ __launch_bounds__(ISS_THREADS) void ivfsq8_select_kernel(IvfBatch a, int k, uint32_t cap, uint32_t Pk, const int64_t *ids,
                                                                    float *out_dist, int64_t *out_labels)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t isq_sel[];
    uint64_t *sh = isq_sel;
    uint64_t *stage = sh + cap;
    SelectScratch &sc = *reinterpret_cast<SelectScratch *>(stage + Pk);
    const int q = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t n = a.seg[(int64_t)q * (a.np + 1) + a.np];
    const uint64_t *keys = a.keys + (int64_t)q * a.pmax;
    auto emit = [&](const uint64_t *sorted, uint32_t nsorted) {
        for (int r = tid; r < k; r += ISS_THREADS) {
            float d = FLT_MAX;
            int64_t lab = -1;
            if ((uint32_t)r < nsorted) {
                const uint64_t e = sorted[r];
                d = (float)(uint32_t)(e >> 32);
                const uint32_t row = (uint32_t)e;
                lab = ids ? ids[row] : (int64_t)row;
            }
            out_dist[(int64_t)q * k + r] = d;
            out_labels[(int64_t)q * k + r] = lab;
        }
    };
    if (n == 0) {
        emit(nullptr, 0);
        return;
    }
    const bool in_lds = n <= cap;
    if (in_lds) {
        const uint32_t P = next_pow2(n); // <= cap: cap is a power of two
        for (uint32_t i = tid; i < P; i += ISS_THREADS) sh[i] = i < n ? keys[i] : kEntryMax;
        __syncthreads();
        if (P <= 2u * Pk) {
            bitonic_sort_u64(sh, P, tid, ISS_THREADS); // kEntryMax padding sorts last
            emit(sh, n < (uint32_t)k ? n : (uint32_t)k);
            return;
        }
    }
    // here n > 2 Pk >= 2 k (a query that does not fit has more than cap >= IVF_SELECT_LDS_KEYS keys)
    const uint64_t *src = in_lds ? sh : keys;
    auto each = [&](auto &&f) {
        for (uint32_t i = tid; i < n; i += ISS_THREADS) f(src[i]);
    };
    if (tid == 0) sc.out_count = 0; // (radix_kth's barriers lie between this and the compaction)
    const uint64_t pivot = radix_kth<ISS_THREADS>(each, (uint32_t)k, sc.radix, tid);
    compact_le<ISS_THREADS>(each, pivot, stage, (uint32_t)k, Pk, &sc.out_count, tid);
    __syncthreads();
    bitonic_sort_u64(stage, Pk, tid, ISS_THREADS);
    emit(stage, (uint32_t)k);
}

void launch_ivfsq8_select(const IvfBatch &a, int k, const int64_t *ids, float *dist, int64_t *labels, hipStream_t s)
{
    if (a.nq <= 0) return;
    const uint32_t Pk = next_pow2_host((uint32_t)k);
    // room for the LDS copy: what the largest query of the handle needs, up to IVF_SELECT_LDS_KEYS
    const uint32_t cap = a.pmax >= (int64_t)IVF_SELECT_LDS_KEYS ? IVF_SELECT_LDS_KEYS : next_pow2_host((uint32_t)std::max<int64_t>(a.pmax, 2));
    const size_t shmem = ((size_t)cap + Pk) * sizeof(uint64_t) + sizeof(SelectScratch);
    allow_big_lds(ivfsq8_select_kernel, shmem); // (at most 148.5 KB of the 160 KB a workgroup may hold)
    hipLaunchKernelGGL(ivfsq8_select_kernel, dim3((unsigned)a.nq), dim3(ISS_THREADS), shmem, s, a, k, cap, Pk, ids, dist, labels);
}

} // namespace lb
