// kernels_ivf.hip -- the IVF-Flat index (ivf.hip; semantics in include/longbow_gpu.h, lb_gpu_ivf_*): the scan of the probed lists,
// the selection of the k smallest of a query's keys, the plan of a batch, the stable counting sort that builds the lists, and the
// segmented compaction that builds the visible lists of a row filter.
//
// The rows stay in insertion order and a list is an ascending array of row numbers, so the list scan is scan_kernel's walk of a
// row list (kernels_scan.hip, MAPPED) with a list per (query, probe slot): each lane owns one row and carries that row's f32
// accumulator chain(s) across D in the reference's order (lb_exact.h), rows staged through LDS in coalesced 16-byte pieces.
// The work lookup and the grid rule are lb_list_scan.h's, shared with the other list scans; the walk over (tile, chunk) is stated
// there too and restated in ivf_scan_kernel for the reason given at its loop.
// Nothing is admitted against a threshold: every scanned row leaves one key, and ivf_select_kernel takes the k smallest.
// No FMA contraction here.
#include "lb_device.h"
#include "lb_exact.h"
#include "lb_ivf.h"
#include "lb_list_scan.h"
#include "lb_select.h"

#include <float.h>
#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

constexpr int IV_ROWS = 128;       // rows per tile == threads per workgroup
constexpr int IV_DK = 64;          // floats per row per stage
constexpr int IV_LD = IV_DK + 4;   // padded LDS row stride (floats): conflict-free ds_read_b128
constexpr int IV_GEN_ROWS = 256;   // rows per tile of the generic form

// Work = (query, probe slot, 128-row tile of that list), found as lb_list_scan.h states and walked as it states, in this
// kernel's own text (below).  A stage is [rows | query chunk] (34.6 KB with the register-held prefetch of the next one, 4
// workgroups per CU).  D % 4 == 0, X and Q 16-byte aligned.
template <int METRIC, int ORDER>
__global__ __launch_bounds__(IV_ROWS) void ivf_scan_kernel(IvfBatch a)
{
    constexpr int STAGE_F = IV_ROWS * IV_LD + IV_DK;
    __shared__ __attribute__((aligned(16))) float lds[STAGE_F];
    ListWork w;
    if (!ivf_list_work(a, IV_ROWS, w)) return;
    const int tid = threadIdx.x;
    const int D = a.D;
    const int nchunks = (D + IV_DK - 1) / IV_DK;
    const uint32_t ntiles = (w.len + IV_ROWS - 1) / IV_ROWS;
    const float *q_src = a.Q + (int64_t)w.q * D;
    const float na = METRIC == METRIC_COS ? a.qna[w.q] : 0.f;

    constexpr int PPR = IV_DK / 4; // 16-byte pieces per row chunk == loads per thread per stage
    const bool q_loader = tid < PPR;
    f32x4 stg[PPR];
    f32x4 stq = {0.f, 0.f, 0.f, 0.f};
    uint32_t rid[PPR]; // the rows behind this thread's PPR staging slots of the tile being loaded
    auto load_stage = [&](uint32_t tile, int c) {
        const uint32_t trow0 = tile * IV_ROWS;
        const int d0 = c * IV_DK;
        if (q_loader) {
            int k = d0 + tid * 4;
            if (k > D - 4) k = D - 4;
            stq = *reinterpret_cast<const f32x4 *>(q_src + k);
        }
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < PPR; i++) {
                uint32_t pos = trow0 + ((uint32_t)(tid + IV_ROWS * i) >> 4);
                if (pos >= w.len) pos = w.len - 1;
                rid[i] = w.rmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int p = (tid + IV_ROWS * i) & (PPR - 1);
            int k = d0 + p * 4;
            if (k > D - 4) k = D - 4; // chunks past D are never consumed
            // (a plain load: other queries of the batch probe the same list and find it in L2 / MALL)
            stg[i] = *reinterpret_cast<const f32x4 *>(a.X + (int64_t)rid[i] * D + k);
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int ch = tid + IV_ROWS * i;
            *reinterpret_cast<f32x4 *>(&lds[(ch >> 4) * IV_LD + (ch & (PPR - 1)) * 4]) = stg[i];
        }
        if (q_loader) *reinterpret_cast<f32x4 *>(&lds[IV_ROWS * IV_LD + tid * 4]) = stq;
    };

    Acc<ORDER> acc; // L2: sum (q-x)^2 ; cos/dot: sum q*x
    Acc<ORDER> nb;  // cos: sum x*x
    // a finished tile's key is written right after the next stage's loads are issued
    float pend_dist = 0.f;
    bool pending = false;
    uint32_t pend_tile = 0;
    auto flush = [&]() {
        const uint32_t pos = pend_tile * IV_ROWS + tid;
        if (pos < w.len) w.out[pos] = pack_entry(pend_dist, w.rmap[pos]);
        pending = false;
    };

    // walk_list_tiles' walk (lb_list_scan.h) in this kernel's own text, kept in step with it by hand.  Built over the shared
    // walk the six instantiations came out 4 - 68 instructions different (same registers, LDS and occupancy), and three of 24
    // scan-slot rows missed the rule of LABNOTES R34.1, each by less than 1 us or 0.3 %: <L2, SEQ> and <cos, SEQ> at 1 query x
    // 8 probes, <dot, UNROLL4> at 1024 x 8.
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
        if (pending) flush();
        if (c == 0) {
            acc.zero();
            nb.zero();
        }
        {
            const float *xr = &lds[tid * IV_LD];
            const float *lq = &lds[IV_ROWS * IV_LD];
            const int d0 = c * IV_DK;
            const int nfull4 = (min(D, d0 + IV_DK) - d0) >> 2;
#pragma unroll 4
            for (int g = 0; g < nfull4; g++) {
                const f32x4 xv = *reinterpret_cast<const f32x4 *>(&xr[g * 4]);
                if (METRIC == METRIC_COS) nb.add4_sq(xv);
                acc.template add4_pair<METRIC>(*reinterpret_cast<const f32x4 *>(&lq[g * 4]), xv);
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (has_next) write_stage();
        if (c == nchunks - 1) {
            pend_dist = exact_distance<METRIC>(acc.total(), nb.total(), na, D, false);
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

// D % 4 != 0 or a misaligned base: one lane per row walks its row straight from global memory.  Same arithmetic.
template <int METRIC, int ORDER>
__global__ __launch_bounds__(IV_GEN_ROWS) void ivf_scan_generic_kernel(IvfBatch a)
{
    ListWork w;
    if (!ivf_list_work(a, IV_GEN_ROWS, w)) return;
    const int D = a.D;
    const float *q = a.Q + (int64_t)w.q * D;
    const float na = METRIC == METRIC_COS ? a.qna[w.q] : 0.f;
    for (uint64_t pos = (uint64_t)blockIdx.x * IV_GEN_ROWS + threadIdx.x; pos < w.len; pos += (uint64_t)gridDim.x * IV_GEN_ROWS) {
        const uint32_t row = w.rmap[pos];
        float t, nbt;
        exact_pair_sums<METRIC, ORDER>(a.X + (int64_t)row * D, q, D, t, nbt);
        w.out[pos] = pack_entry(exact_distance<METRIC>(t, nbt, na, D, false), row);
    }
}

void launch_ivf_scan(int metric, int order, const IvfBatch &a, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.nq * a.np;
    if (pairs <= 0 || maxlen <= 0) return;
    const bool staged = a.D % 4 == 0 && ((reinterpret_cast<uintptr_t>(a.X) | reinterpret_cast<uintptr_t>(a.Q)) & 15) == 0;
    const dim3 grid = ivf_scan_grid(pairs, maxlen, staged ? IV_ROWS : IV_GEN_ROWS);
    with_metric_order(metric, order, [&](auto m, auto o) {
        if (staged) hipLaunchKernelGGL((ivf_scan_kernel<decltype(m)::value, decltype(o)::value>), grid, dim3(IV_ROWS), 0, s, a);
        else hipLaunchKernelGGL((ivf_scan_generic_kernel<decltype(m)::value, decltype(o)::value>), grid, dim3(IV_GEN_ROWS), 0, s, a);
    });
}

// ---- plan -----------------------------------------------------------------------------------------------------------------
// One wave per query: seg[q][p] = rows of the probed lists before slot p, seg[q][np] = P_q; the search's counters.
__global__ __launch_bounds__(64) void ivf_plan_kernel(IvfBatch a, unsigned long long *stats)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    uint32_t *seg = a.seg + (int64_t)q * (a.np + 1);
    uint64_t run = 0;
    for (int p0 = 0; p0 < a.np; p0 += 64) {
        const int p = p0 + lane;
        uint32_t len = 0;
        if (p < a.np) {
            const int64_t l = a.probes[(int64_t)q * a.np + p];
            if (l >= 0 && l < a.L.nlist) len = a.L.off[l + 1] - a.L.off[l];
        }
        const uint32_t incl = wave_incl_scan(len, lane); // (distinct lists: at most the handle's rows, < 2^31)
        if (p < a.np) seg[p] = (uint32_t)std::min<uint64_t>(run + incl - len, 0xffffffffull);
        run += __shfl(incl, 63);
    }
    if (lane == 0) {
        const uint32_t total = (uint32_t)std::min<uint64_t>(run, (uint64_t)a.pmax);
        seg[a.np] = total;
        atomicAdd(&stats[1], (unsigned long long)total);
        atomicMax(&stats[2], (unsigned long long)total);
        if (total <= IVF_SELECT_LDS_KEYS) atomicAdd(&stats[3], 1ull);
    }
}

// every list probed, in list order: what the coarse search's labels are as a set when np == nlist
__global__ void ivf_all_probes_kernel(int64_t *probes, int64_t total, int np)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) probes[i] = i % np;
}

void launch_ivf_all_probes(int64_t *probes, int nq, int np, hipStream_t s)
{
    const int64_t total = (int64_t)nq * np;
    if (total <= 0) return;
    hipLaunchKernelGGL(ivf_all_probes_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, probes, total, np);
}

void launch_ivf_plan(const IvfBatch &a, unsigned long long *stats, hipStream_t s)
{
    if (a.nq <= 0) return;
    hipLaunchKernelGGL(ivf_plan_kernel, dim3((unsigned)a.nq), dim3(64), 0, s, a, stats);
}

// ---- select ---------------------------------------------------------------------------------------------------------------
// One workgroup per query: the k smallest of its n = P_q unique u64 keys, ascending (select_kernel's method, kernels_select.hip).
//   n <= cap (the LDS copy's room): the keys are copied to LDS; with next_pow2(n) <= 2 Pk a bitonic sort of everything,
//   otherwise, and for every n > cap: MSB radix select of the k-th smallest key (8 bits a pass; the counting passes read the LDS
//   copy, or the keys in global memory when they do not fit), compaction of the k keys at or below it into LDS, a sort of those.
// Keys are unique (the row is part of the key), so exactly k keys are at or below the pivot.
// LDS: keys u64[cap] | stage u64[Pk] | hist u32[256] | wave sums u32[4] | scalars u32[8]
// (the tail has SelectScratch's size.)  This kernel keeps its own text of the radix walk, the compaction and the emit, in step
// with lb_select.h's radix_kth / compact_le / emit_sorted by hand.  Its time depends on where its three loops over the keys fall
// in the code: this very text with the loops moved by 12, 40 or 52 bytes is 1 - 3 % slower, by 24 bytes it is level.  Built over
// the shared pieces the loops came out instruction for instruction the same but elsewhere, in every arrangement tried on a slow
// spot (0.7 - 2 % on the select slot).  Until the loops are made indifferent to their placement, the text stays (LABNOTES R23.1).
constexpr int IVS_THREADS = 1024;

__global__ __launch_bounds__(IVS_THREADS) void ivf_select_kernel(IvfBatch a, int k, uint32_t cap, uint32_t Pk, const int64_t *ids,
                                                                 float *out_dist, int64_t *out_labels)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t sh[];
    uint64_t *stage = sh + cap;
    uint32_t *hist = reinterpret_cast<uint32_t *>(stage + Pk);
    uint32_t *wsum = hist + 256;
    uint32_t *scal = wsum + 4; // [0] = bucket, [1] = need, [2] = compaction counter, [4] = take the whole bucket
    const int q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = a.seg[(int64_t)q * (a.np + 1) + a.np];
    const uint64_t *keys = a.keys + (int64_t)q * a.pmax;
    auto emit = [&](const uint64_t *sorted, uint32_t nsorted) {
        for (int r = tid; r < k; r += IVS_THREADS) {
            float d = FLT_MAX;
            int64_t lab = -1;
            if ((uint32_t)r < nsorted) {
                const uint64_t e = sorted[r];
                d = entry_key(e);
                const uint32_t row = entry_row(e);
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
        for (uint32_t i = tid; i < P; i += IVS_THREADS) sh[i] = i < n ? keys[i] : kEntryMax;
        __syncthreads();
        if (P <= 2u * Pk) {
            bitonic_sort_u64(sh, P, tid, IVS_THREADS); // kEntryMax padding sorts last
            emit(sh, n < (uint32_t)k ? n : (uint32_t)k);
            return;
        }
    }
    // here n > 2 Pk >= 2 k (a query that does not fit has more than cap >= IVF_SELECT_LDS_KEYS keys)
    const uint64_t *src = in_lds ? sh : keys;

    // ---- radix select of the k-th smallest (1-based rank `need`) ----
    // Leading bytes shared by every key (distances live in a narrow range) need no pass.
    unsigned long long *red = reinterpret_cast<unsigned long long *>(hist); // [0] = OR, [1] = AND of the keys
    if (tid == 0) {
        red[0] = 0ull;
        red[1] = ~0ull;
        scal[2] = 0;
    }
    __syncthreads();
    {
        uint64_t o = 0, an = ~0ull;
        for (uint32_t i = tid; i < n; i += IVS_THREADS) {
            const uint64_t e = src[i];
            o |= e;
            an &= e;
        }
        wave_or_and_u64(o, an); // one pair of LDS atomics per wave
        if (lane == 63) {
            atomicOr(&red[0], (unsigned long long)o);
            atomicAnd(&red[1], (unsigned long long)an);
        }
    }
    __syncthreads();
    const uint64_t diff = red[0] ^ red[1]; // bit positions that differ among the keys (never 0: n >= 2 unique keys)
    const uint64_t common = red[1];
    __syncthreads();
    int first_shift = 56;
    uint64_t prefix = 0, mask = 0;
    if (diff != 0ull) {
        const int same_bytes = __builtin_clzll(diff) >> 3; // whole leading bytes identical
        first_shift = 56 - 8 * same_bytes;
        if (same_bytes > 0) {
            mask = ~0ull << (64 - 8 * same_bytes);
            prefix = common & mask;
        }
    }
    uint32_t need = (uint32_t)k;
    for (int shift = first_shift; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += IVS_THREADS) {
            const uint64_t e = src[i];
            if ((e & mask) == prefix) atomicAdd(&hist[(uint32_t)(e >> shift) & 0xffu], 1u);
        }
        __syncthreads();
        const uint32_t h = tid < 256 ? hist[tid] : 0u;
        uint32_t incl = wave_incl_scan(h, lane);
        if (tid < 256 && lane == 63) wsum[wave] = incl;
        __syncthreads();
        if (tid < 256) {
            uint32_t base = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) base += (w < wave) ? wsum[w] : 0u;
            incl += base;
            const uint32_t excl = incl - h;
            if (excl < need && need <= incl) {
                scal[0] = (uint32_t)tid;
                scal[1] = need - excl;
                scal[4] = (need == incl) ? 1u : 0u; // the whole bucket is wanted: no need to split it further
            }
        }
        __syncthreads();
        prefix |= (uint64_t)scal[0] << shift;
        mask |= 0xffull << shift;
        need = scal[1];
        const bool whole_bucket = scal[4] != 0u;
        __syncthreads();
        if (whole_bucket) {
            prefix |= ~mask; // every key sharing the resolved bytes is kept
            break;
        }
    }
    const uint64_t pivot = prefix; // >= the k-th smallest key and < the (k+1)-th: exactly k keys are <= pivot
    for (uint32_t i = tid; i < n; i += IVS_THREADS) {
        const uint64_t e = src[i];
        if (e <= pivot) {
            const uint32_t pos = atomicAdd(&scal[2], 1u);
            if (pos < Pk) stage[pos] = e; // pos < k by construction
        }
    }
    for (uint32_t i = (uint32_t)k + tid; i < Pk; i += IVS_THREADS) stage[i] = kEntryMax;
    __syncthreads();
    bitonic_sort_u64(stage, Pk, tid, IVS_THREADS);
    emit(stage, (uint32_t)k);
}

void launch_ivf_select(const IvfBatch &a, int k, const int64_t *ids, float *dist, int64_t *labels, hipStream_t s)
{
    if (a.nq <= 0) return;
    const uint32_t Pk = next_pow2_host((uint32_t)k);
    // room for the LDS copy: what the largest query of the handle needs, up to IVF_SELECT_LDS_KEYS
    const uint32_t cap = a.pmax >= (int64_t)IVF_SELECT_LDS_KEYS ? IVF_SELECT_LDS_KEYS : next_pow2_host((uint32_t)std::max<int64_t>(a.pmax, 2));
    const size_t shmem = ((size_t)cap + Pk) * sizeof(uint64_t) + sizeof(SelectScratch);
    allow_big_lds(ivf_select_kernel, shmem); // (at most 148.5 KB of the 160 KB a workgroup may hold)
    hipLaunchKernelGGL(ivf_select_kernel, dim3((unsigned)a.nq), dim3(IVS_THREADS), shmem, s, a, k, cap, Pk, ids, dist, labels);
}

// ---- the lists: a stable counting sort of the rows by list ----------------------------------------------------------------
// Rows are cut into chunks; hist[chunk][list] counts, becomes the exclusive prefix over the chunks per list, and then the
// cursor of the chunk's wave, which places its rows in row order.  Integer only.
struct IvfSort {
    const uint32_t *assign;
    int64_t n, chunk_rows, nchunks;
    int nlist;
    uint32_t *hist; // [nchunks][nlist]
    uint32_t *off;  // [nlist + 1]
    uint32_t *rows; // [n]
};

// at most 1024 chunks of at least 4096 rows, and at most 2^24 counters
static void ivf_sort_shape(int64_t n, int nlist, int64_t *chunk_rows, int64_t *nchunks)
{
    int64_t cr = std::max<int64_t>(4096, (n + 1023) / 1024);
    const int64_t max_chunks = std::max<int64_t>(1, ((int64_t)1 << 24) / nlist);
    cr = std::max<int64_t>(cr, (n + max_chunks - 1) / max_chunks);
    cr = (cr + 63) & ~(int64_t)63;
    *chunk_rows = cr;
    *nchunks = std::max<int64_t>(1, (n + cr - 1) / cr);
}

size_t ivf_sort_hist_words(int64_t n, int nlist)
{
    int64_t cr, nc;
    ivf_sort_shape(n, nlist, &cr, &nc);
    return (size_t)nc * (size_t)nlist;
}

__global__ void ivf_narrow_kernel(const int64_t *labels, int64_t n, uint32_t *assign)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        assign[i] = (uint32_t)labels[i];
}

void launch_ivf_narrow(const int64_t *labels, int64_t n, uint32_t *assign, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(ivf_narrow_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, labels, n, assign);
}

__global__ __launch_bounds__(256) void ivf_hist_kernel(IvfSort a)
{
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk_rows;
    const int64_t r1 = r0 + a.chunk_rows < a.n ? r0 + a.chunk_rows : a.n;
    uint32_t *h = a.hist + (int64_t)blockIdx.x * a.nlist;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
        const uint32_t key = a.assign[r];
        if (key < (uint32_t)a.nlist) atomicAdd(&h[key], 1u);
    }
}

// thread = list: the column of chunk counts becomes its exclusive prefix, the total goes to off[list]
__global__ __launch_bounds__(256) void ivf_colscan_kernel(IvfSort a)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= a.nlist) return;
    uint32_t run = 0;
    for (int64_t ch = 0; ch < a.nchunks; ch++) {
        uint32_t *h = a.hist + ch * a.nlist + l;
        const uint32_t v = *h;
        *h = run;
        run += v;
    }
    a.off[l] = run;
}

// one workgroup: off[0 .. nlist) sizes -> their exclusive prefix, off[nlist] = the total
__global__ __launch_bounds__(1024) void ivf_offsets_kernel(uint32_t *off, int nlist)
{
    __shared__ uint32_t s_scan[1024];
    const int t = threadIdx.x;
    const int per = (nlist + 1023) / 1024;
    const int b = t * per, e = b + per < nlist ? b + per : nlist;
    uint32_t sum = 0;
    for (int i = b; i < e; i++) sum += off[i];
    s_scan[t] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t add = t >= o ? s_scan[t - o] : 0u;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    uint32_t run = s_scan[t] - sum;
    for (int i = b; i < e; i++) {
        const uint32_t v = off[i];
        off[i] = run;
        run += v;
    }
    if (t == 1023) off[nlist] = s_scan[1023];
}

// One wave per chunk, 64 rows at a time in row order.  A lane's place is its list's cursor plus the number of lower lanes with
// the same list (sixteen ballots, one per bit of the list number); the last such lane moves the cursor.  The cursors are the
// chunk's own row of hist, in global memory (65,536 lists do not fit LDS): this wave alone touches them, through device-scope
// atomic loads and stores with a fence between the steps.
__global__ __launch_bounds__(64) void ivf_scatter_kernel(IvfSort a)
{
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk_rows;
    const int64_t r1 = r0 + a.chunk_rows < a.n ? r0 + a.chunk_rows : a.n;
    uint32_t *cur = a.hist + (int64_t)blockIdx.x * a.nlist;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t b = r0; b < r1; b += 64) {
        const int64_t row = b + lane;
        uint32_t key = row < r1 ? a.assign[row] : 0xffffffffu;
        const bool valid = key < (uint32_t)a.nlist;
        if (!valid) key = 0;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 16; bit++) {
            const unsigned long long bal = __ballot(valid && ((key >> bit) & 1u));
            peers &= ((key >> bit) & 1u) ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lt), cnt = (uint32_t)__popcll(peers);
        if (valid) {
            const uint32_t base = __hip_atomic_load(&cur[key], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t at = (uint64_t)a.off[key] + base + rank;
            if (at < (uint64_t)a.n) a.rows[at] = (uint32_t)row;
            if (rank == cnt - 1) __hip_atomic_store(&cur[key], base + cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __threadfence(); // the cursors of this step are in place before the next step reads them
    }
}

hipError_t launch_ivf_sort(const uint32_t *assign, int64_t n, int nlist, uint32_t *hist, uint32_t *off, uint32_t *rows, hipStream_t s)
{
    IvfSort a{};
    a.assign = assign;
    a.n = n;
    a.nlist = nlist;
    ivf_sort_shape(n, nlist, &a.chunk_rows, &a.nchunks);
    a.hist = hist;
    a.off = off;
    a.rows = rows;
    const hipError_t e = hipMemsetAsync(hist, 0, (size_t)a.nchunks * nlist * 4, s);
    if (e != hipSuccess) return e; // stale cursors would misplace rows: nothing is launched
    if (n > 0) hipLaunchKernelGGL(ivf_hist_kernel, dim3((unsigned)a.nchunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ivf_colscan_kernel, dim3((unsigned)((nlist + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ivf_offsets_kernel, dim3(1), dim3(1024), 0, s, off, nlist);
    if (n > 0) hipLaunchKernelGGL(ivf_scatter_kernel, dim3((unsigned)a.nchunks), dim3(64), 0, s, a);
    return hipSuccess;
}

// ---- the visible lists: a segmented compaction of the lists under a row mask ------------------------------------------------
// The n list positions are walked as one array, VIS_ROWS to a workgroup and eight to a thread, so every list keeps its order.
//   count    bit i of a thread's byte = mask[rows[position i]] != 0 (the only gather); the byte is kept, the workgroup's sum too
//   offsets  launch_compact_offsets over the workgroups' sums
//   place    the visible rows of each workgroup (POS: their positions instead, which need no load) go behind those before it; in
//            the same launch one wave per list boundary
//            counts the visible positions below off[l]: the sum of the workgroups before its own, plus the bits below it in that
//            workgroup's 64 words (a lane a word)
// Integer only; no workgroup waits for another.
constexpr int VIS_THREADS = 256;
constexpr int VIS_PER = 8;
constexpr int VIS_ROWS = VIS_THREADS * VIS_PER;
constexpr int VIS_WORDS = VIS_ROWS / 32; // == 64: one wave reads a workgroup's bits

struct IvfVisible {
    const uint8_t *mask; // [n]
    IvfLists L;          // the lists of all n rows
    int64_t n, nblk;
    uint32_t *blk;       // [nblk + 1]: visible positions per workgroup, then their exclusive prefix and the total
    uint32_t *bits;      // [nblk][VIS_WORDS]: position p is bit p % 32 of word p / 32; positions past n are 0
    uint32_t *voff;      // [nlist + 1]
    uint32_t *vrows;     // [n]: the visible rows, or their positions in L.rows
};

// the sum of v over the workgroup's four waves, in every thread; `before`: the sum over the waves below this one
__device__ __forceinline__ uint32_t vis_block_sum(uint32_t wave_total, uint32_t *s_wave, uint32_t &before)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) s_wave[wave] = wave_total;
    __syncthreads();
    uint32_t tot = 0;
    before = 0;
#pragma unroll
    for (int w = 0; w < VIS_THREADS / 64; w++) {
        const uint32_t t = s_wave[w];
        if (w < wave) before += t;
        tot += t;
    }
    return tot;
}

// the eight rows at positions [base, base + 8), base % 8 == 0 and base + 8 <= n (rows is 32-byte aligned)
__device__ __forceinline__ void vis_load8(const uint32_t *rows, int64_t base, uint32_t r[VIS_PER])
{
    const uint4 a = *reinterpret_cast<const uint4 *>(rows + base), b = *reinterpret_cast<const uint4 *>(rows + base + 4);
    r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w;
    r[4] = b.x, r[5] = b.y, r[6] = b.z, r[7] = b.w;
}

__global__ __launch_bounds__(VIS_THREADS) void ivf_visible_count_kernel(IvfVisible a)
{
    __shared__ uint32_t s_wave[VIS_THREADS / 64];
    const int64_t t = (int64_t)blockIdx.x * VIS_THREADS + threadIdx.x, base = t * VIS_PER;
    uint32_t b = 0;
    if (base + VIS_PER <= a.n) {
        uint32_t r[VIS_PER];
        vis_load8(a.L.rows, base, r);
#pragma unroll
        for (int i = 0; i < VIS_PER; i++)
            if ((int64_t)r[i] < a.n && a.mask[r[i]]) b |= 1u << i;
    } else {
        for (int i = 0; i < VIS_PER && base + i < a.n; i++) {
            const uint32_t r = a.L.rows[base + i];
            if ((int64_t)r < a.n && a.mask[r]) b |= 1u << i;
        }
    }
    reinterpret_cast<uint8_t *>(a.bits)[t] = (uint8_t)b; // (every thread of the grid: the bytes past n are zero)
    uint32_t before;
    const uint32_t tot = vis_block_sum(wave_incl_scan((uint32_t)__popc(b), threadIdx.x & 63), s_wave, before);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = tot;
}

// workgroups [0, nblk) place the rows; the ones behind them take four list boundaries each, a wave a boundary
template <bool POS>
__global__ __launch_bounds__(VIS_THREADS) void ivf_visible_place_kernel(IvfVisible a)
{
    __shared__ uint32_t s_wave[VIS_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int64_t)blockIdx.x >= a.nblk) {
        const int64_t l = ((int64_t)blockIdx.x - a.nblk) * (VIS_THREADS / 64) + wave;
        if (l > a.L.nlist) return;
        const int64_t p = std::min<int64_t>(a.L.off[l], a.n);
        const int64_t blk = p / VIS_ROWS; // <= nblk
        const uint32_t w = (uint32_t)(p % VIS_ROWS), lo = (uint32_t)lane * 32u;
        uint32_t c = 0;
        if (blk < a.nblk) { // (else p == n at the end of the last workgroup: blk[nblk] is the answer)
            const uint32_t below = w >= lo + 32u ? 0xffffffffu : w > lo ? (1u << (w - lo)) - 1u : 0u;
            c = (uint32_t)__popc(a.bits[blk * VIS_WORDS + lane] & below);
        }
        c = wave_incl_scan(c, lane);
        if (lane == 63) a.voff[l] = a.blk[blk] + c;
        return;
    }
    const int64_t t = (int64_t)blockIdx.x * VIS_THREADS + threadIdx.x, base = t * VIS_PER;
    const uint32_t b = reinterpret_cast<const uint8_t *>(a.bits)[t];
    const uint32_t c = (uint32_t)__popc(b);
    const uint32_t incl = wave_incl_scan(c, lane);
    uint32_t before;
    (void)vis_block_sum(incl, s_wave, before);
    if (b == 0) return;
    uint64_t at = (uint64_t)a.blk[blockIdx.x] + before + incl - c;
    if (POS) {
        for (int i = 0; i < VIS_PER; i++)
            if ((b >> i) & 1u) { // (set only for positions below n < 2^31)
                if (at < (uint64_t)a.n) a.vrows[at] = (uint32_t)(base + i);
                at++;
            }
    } else if (base + VIS_PER <= a.n) {
        uint32_t r[VIS_PER];
        vis_load8(a.L.rows, base, r);
#pragma unroll
        for (int i = 0; i < VIS_PER; i++)
            if ((b >> i) & 1u) {
                if (at < (uint64_t)a.n) a.vrows[at] = r[i];
                at++;
            }
    } else {
        for (int i = 0; i < VIS_PER; i++)
            if ((b >> i) & 1u) { // (set only for positions below n)
                if (at < (uint64_t)a.n) a.vrows[at] = a.L.rows[base + i];
                at++;
            }
    }
}

static int64_t vis_blocks(int64_t n) { return (n + VIS_ROWS - 1) / VIS_ROWS; }
static size_t vis_bits_at(int64_t nb) { return (((size_t)nb + 1) * 4 + 15) & ~(size_t)15; } // behind blk, 16-byte aligned

size_t ivf_visible_scratch_bytes(int64_t n)
{
    const int64_t nb = vis_blocks(n);
    return vis_bits_at(nb) + (size_t)nb * VIS_WORDS * 4;
}

hipError_t launch_ivf_visible(const uint8_t *mask, const IvfLists &L, int64_t n, bool positions, void *scratch, uint32_t *voff, uint32_t *vrows,
                              hipStream_t s)
{
    if (n <= 0) return hipMemsetAsync(voff, 0, ((size_t)L.nlist + 1) * 4, s);
    IvfVisible a{};
    a.mask = mask;
    a.L = L;
    a.n = n;
    a.nblk = vis_blocks(n);
    a.blk = static_cast<uint32_t *>(scratch);
    a.bits = reinterpret_cast<uint32_t *>(static_cast<char *>(scratch) + vis_bits_at(a.nblk));
    a.voff = voff;
    a.vrows = vrows;
    const int64_t bounds = ((int64_t)L.nlist + 1 + VIS_THREADS / 64 - 1) / (VIS_THREADS / 64);
    hipLaunchKernelGGL(ivf_visible_count_kernel, dim3((unsigned)a.nblk), dim3(VIS_THREADS), 0, s, a);
    launch_compact_offsets(a.blk, a.nblk, s);
    if (positions) hipLaunchKernelGGL(ivf_visible_place_kernel<true>, dim3((unsigned)(a.nblk + bounds)), dim3(VIS_THREADS), 0, s, a);
    else hipLaunchKernelGGL(ivf_visible_place_kernel<false>, dim3((unsigned)(a.nblk + bounds)), dim3(VIS_THREADS), 0, s, a);
    return hipSuccess;
}

} // namespace lb
