// kernels_refine.hip -- the device side of lb_gpu_index_refine (refine.hip; semantics in include/longbow_gpu.h): nq shortlists of
// c candidate rows each become, per query, the ascending list of the distinct valid rows (refine_prepare_kernel) and one key per
// list position (refine_scan_kernel); launch_ivf_select (kernels_ivf.hip) then takes the k smallest keys of every query.
//
// The scan is ivf_scan_kernel's method (kernels_ivf.hip) over these per-query lists, on the walk and the grid rule that
// lb_list_scan.h states for every list scan: each lane owns one row and carries that row's f32 accumulator chain(s) across D in
// the reference's order (lb_exact.h), rows staged through LDS in coalesced 16-byte pieces; the rows of a float16 index are
// widened to f32 (exact) as the stage is written, as scan_kernel does (kernels_scan.hip).  Every list position leaves one key.
// Plain vector loads and stores, no atomics, no workgroup waits for another.
// No FMA contraction here.
#include "lb_device.h"
#include "lb_exact.h"
#include "lb_list_scan.h"
#include "lb_refine.h"
#include "lb_select.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

constexpr int RF_ROWS = 128;     // rows per tile == threads per workgroup
constexpr int RF_DK = 64;        // row elements per stage
constexpr int RF_LD = RF_DK + 4; // padded LDS row stride (floats): conflict-free ds_read_b128
constexpr int RF_GEN_ROWS = 256; // rows per tile of the generic form
constexpr uint32_t RF_NONE = 0xffffffffu; // an entry outside [0, ntotal): no row (an index holds at most 2^32 - 1 rows)

// ---- prepare --------------------------------------------------------------------------------------------------------------
// In-LDS bitonic sort of P (power of two) u32 values, ascending, by the whole workgroup (bitonic_sort_u64's walk, lb_select.h).
__device__ __forceinline__ void bitonic_sort_u32(uint32_t *sh, uint32_t P, int tid, int nthreads)
{
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (P >> 1); t += nthreads) {
                const uint32_t i = 2 * t - (t & (j - 1));
                const uint32_t l = i + j;
                const uint32_t a = sh[i], b = sh[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    sh[i] = b;
                    sh[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

// One workgroup per query: the c entries, those outside [0, ntotal) or removed (a.live) as RF_NONE, are sorted in LDS (P = next_pow2(c) words, RF_NONE
// sorts last); a position is kept when it holds a row and differs from the one before it; the kept ones go to list[q] in order,
// each thread placing the run of positions it owns behind the count of those before it.  len[q] <= c.
// LDS: u32[P] | wave sums u32[NT / 64]
template <int NT>
__global__ __launch_bounds__(NT) void refine_prepare_kernel(RefineBatch a, uint32_t P)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t rsh[];
    uint32_t *wsum = rsh + P;
    const int q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t *rows = a.rows + (int64_t)q * a.c;
    for (uint32_t i = tid; i < P; i += NT) {
        uint32_t v = RF_NONE;
        if (i < (uint32_t)a.c) {
            const int64_t r = rows[i];
            if (r >= 0 && r < a.ntotal && (!a.live || a.live[r])) v = (uint32_t)r;
        }
        rsh[i] = v;
    }
    __syncthreads();
    bitonic_sort_u32(rsh, P, tid, NT);
    const uint32_t per = P > (uint32_t)NT ? P / NT : 1u; // positions per thread (both are powers of two)
    const uint32_t b = (uint32_t)tid * per;
    const uint32_t e = b + per < P ? b + per : P;
    auto kept = [&](uint32_t i) {
        const uint32_t v = rsh[i];
        return v != RF_NONE && (i == 0 || v != rsh[i - 1]);
    };
    uint32_t cnt = 0;
    for (uint32_t i = b; i < e; i++) cnt += kept(i) ? 1u : 0u;
    const uint32_t incl = wave_incl_scan(cnt, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
        const uint32_t t = wsum[w];
        if (w < wave) before += t;
        total += t;
    }
    uint32_t at = before + incl - cnt;
    uint32_t *list = a.list + (int64_t)q * a.c;
    for (uint32_t i = b; i < e; i++)
        if (kept(i)) {
            if (at < (uint32_t)a.c) list[at] = rsh[i]; // (always: at most c positions hold a row)
            at++;
        }
    if (tid == 0) a.len[q] = total < (uint32_t)a.c ? total : (uint32_t)a.c;
}

void launch_refine_prepare(const RefineBatch &a, hipStream_t s)
{
    if (a.nq <= 0 || a.c <= 0) return;
    const uint32_t P = next_pow2_host((uint32_t)std::max(a.c, 2));
    if (P <= 2048) {
        const size_t shmem = ((size_t)P + 256 / 64) * sizeof(uint32_t);
        hipLaunchKernelGGL(refine_prepare_kernel<256>, dim3((unsigned)a.nq), dim3(256), shmem, s, a, P);
    } else {
        const size_t shmem = ((size_t)P + 1024 / 64) * sizeof(uint32_t); // at most 64 KB + 64 B
        allow_big_lds(refine_prepare_kernel<1024>, shmem);
        hipLaunchKernelGGL(refine_prepare_kernel<1024>, dim3((unsigned)a.nq), dim3(1024), shmem, s, a, P);
    }
}

// ---- scan -----------------------------------------------------------------------------------------------------------------
// one 16-byte load of row elements: four f32, or eight fp16
template <typename T> struct RefinePiece { typedef f32x4 type; };
template <> struct RefinePiece<_Float16> { typedef f16x8 type; };

// What a workgroup of the scan works on: query blockIdx.y (wave-uniform).  false: nothing to do.
struct RefineWork {
    uint32_t len;         // rows of the query's list, <= c
    const uint32_t *rmap; // the list, ascending, every row < ntotal
    uint64_t *out;        // the query's keys
};
__device__ __forceinline__ bool refine_work(const RefineBatch &a, int tile_rows, int q, RefineWork &w)
{
    uint32_t len = a.len[q];
    if (len > (uint32_t)a.c) len = (uint32_t)a.c;
    if ((uint64_t)blockIdx.x * (uint32_t)tile_rows >= len) return false; // (an empty list among them)
    w.len = len;
    w.rmap = a.list + (int64_t)q * a.c;
    w.out = a.keys + (int64_t)q * a.c;
    return true;
}

// Work = (query, 128-row tile of its list), walked as lb_list_scan.h states, in this kernel's own text (below).  A stage is [rows | query chunk] of f32 (34.3 KB
// with the register-held prefetch of the next one, 4 workgroups per CU).  D % 4 == 0 (f32 rows) or D % 8 == 0 (fp16 rows), X and
// Q 16-byte aligned.
template <typename T, int METRIC, int ORDER>
__global__ __launch_bounds__(RF_ROWS) void refine_scan_kernel(RefineBatch a)
{
    constexpr int STAGE_F = RF_ROWS * RF_LD + RF_DK;
    __shared__ __attribute__((aligned(16))) float lds[STAGE_F];
    const int q = blockIdx.y;
    RefineWork w;
    if (!refine_work(a, RF_ROWS, q, w)) return;
    const int tid = threadIdx.x;
    const int D = a.D;
    const int nchunks = (D + RF_DK - 1) / RF_DK;
    const uint32_t ntiles = (w.len + RF_ROWS - 1) / RF_ROWS;
    const T *X = static_cast<const T *>(a.X);
    const float *q_src = a.Q + (int64_t)q * D;
    const float na = METRIC == METRIC_COS ? a.qna[q] : 0.f;

    constexpr int EPP = 16 / (int)sizeof(T); // row elements per 16-byte piece
    constexpr int PPR = RF_DK / EPP;         // pieces per row chunk == loads per thread per stage
    constexpr int PSH = PPR == 16 ? 4 : 3;   // log2(PPR)
    typedef typename RefinePiece<T>::type Piece;
    const bool q_loader = tid < RF_DK / 4;
    Piece stg[PPR];
    f32x4 stq = {0.f, 0.f, 0.f, 0.f};
    uint32_t rid[PPR]; // the rows behind this thread's PPR staging slots of the tile being loaded
    auto load_stage = [&](uint32_t tile, int c) {
        const uint32_t trow0 = tile * RF_ROWS;
        const int d0 = c * RF_DK;
        if (q_loader) {
            int k = d0 + tid * 4;
            if (k > D - 4) k = D - 4;
            stq = *reinterpret_cast<const f32x4 *>(q_src + k);
        }
        if (c == 0) {
#pragma unroll
            for (int i = 0; i < PPR; i++) {
                uint32_t pos = trow0 + ((uint32_t)(tid + RF_ROWS * i) >> PSH);
                if (pos >= w.len) pos = w.len - 1;
                rid[i] = w.rmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int p = (tid + RF_ROWS * i) & (PPR - 1);
            int k = d0 + p * EPP;
            if (k > D - EPP) k = D - EPP; // chunks past D are never consumed
            // (a plain load: the shortlists of a batch share rows, which the later queries find in L2 / MALL)
            stg[i] = *reinterpret_cast<const Piece *>(X + (int64_t)rid[i] * D + k);
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < PPR; i++) {
            const int ch = tid + RF_ROWS * i;
            const int r = ch >> PSH, p = ch & (PPR - 1);
            if constexpr (EPP == 4) {
                *reinterpret_cast<f32x4 *>(&lds[r * RF_LD + p * 4]) = stg[i];
            } else {
                const f32x4 lo = {(float)stg[i][0], (float)stg[i][1], (float)stg[i][2], (float)stg[i][3]};
                const f32x4 hi = {(float)stg[i][4], (float)stg[i][5], (float)stg[i][6], (float)stg[i][7]};
                *reinterpret_cast<f32x4 *>(&lds[r * RF_LD + p * 8]) = lo;
                *reinterpret_cast<f32x4 *>(&lds[r * RF_LD + p * 8 + 4]) = hi;
            }
        }
        if (q_loader) *reinterpret_cast<f32x4 *>(&lds[RF_ROWS * RF_LD + tid * 4]) = stq;
    };

    Acc<ORDER> acc; // L2: sum (q-x)^2 ; cos/dot: sum q*x
    Acc<ORDER> nb;  // cos: sum x*x
    // a finished tile's key is written right after the next stage's loads are issued
    float pend_dist = 0.f;
    bool pending = false;
    uint32_t pend_tile = 0;
    auto flush = [&]() {
        const uint32_t pos = pend_tile * RF_ROWS + tid;
        if (pos < w.len) w.out[pos] = pack_entry(pend_dist, w.rmap[pos]);
        pending = false;
    };

    // walk_list_tiles' walk (lb_list_scan.h) in this kernel's own text, kept in step with it by hand.  Built over the shared
    // walk <cos, UNROLL4> took 30 more VGPRs (176 -> 206 on f32 rows, 120 -> 150 on fp16 rows) and its scan slot was 8 - 10 %
    // slower (fp16 rows at 1 and at 1024 queries, f32 rows at 1 query); four more of the twelve instantiations missed the rule
    // of LABNOTES R34.1 by 0.4 - 2.4 %.
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
            const float *xr = &lds[tid * RF_LD];
            const float *lq = &lds[RF_ROWS * RF_LD];
            const int d0 = c * RF_DK;
            const int nfull4 = (min(D, d0 + RF_DK) - d0) >> 2;
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

// Any D, any alignment: one lane per row walks its row straight from global memory.  Same arithmetic.
template <typename T, int METRIC, int ORDER>
__global__ __launch_bounds__(RF_GEN_ROWS) void refine_scan_generic_kernel(RefineBatch a)
{
    const int q = blockIdx.y;
    RefineWork w;
    if (!refine_work(a, RF_GEN_ROWS, q, w)) return;
    const int D = a.D;
    const T *X = static_cast<const T *>(a.X);
    const float *qv = a.Q + (int64_t)q * D;
    const float na = METRIC == METRIC_COS ? a.qna[q] : 0.f;
    for (uint32_t pos = blockIdx.x * RF_GEN_ROWS + threadIdx.x; pos < w.len; pos += gridDim.x * RF_GEN_ROWS) {
        const uint32_t row = w.rmap[pos];
        float t, nbt;
        exact_pair_sums<METRIC, ORDER>(X + (int64_t)row * D, qv, D, t, nbt);
        w.out[pos] = pack_entry(exact_distance<METRIC>(t, nbt, na, D, false), row);
    }
}

template <typename T>
static void launch_refine_scan_t(int metric, int order, const RefineBatch &a, hipStream_t s)
{
    const bool staged = a.D % (16 / (int)sizeof(T)) == 0 && ((reinterpret_cast<uintptr_t>(a.X) | reinterpret_cast<uintptr_t>(a.Q)) & 15) == 0;
    // tiles of a query's list along x (list_scan_gx), queries along y (a batch holds at most 1024)
    const int rows = staged ? RF_ROWS : RF_GEN_ROWS;
    const dim3 grid((unsigned)list_scan_gx(a.nq, ((int64_t)a.c + rows - 1) / rows), (unsigned)a.nq, 1);
    with_metric_order(metric, order, [&](auto m, auto o) {
        if (staged) hipLaunchKernelGGL((refine_scan_kernel<T, decltype(m)::value, decltype(o)::value>), grid, dim3(RF_ROWS), 0, s, a);
        else hipLaunchKernelGGL((refine_scan_generic_kernel<T, decltype(m)::value, decltype(o)::value>), grid, dim3(RF_GEN_ROWS), 0, s, a);
    });
}

void launch_refine_scan(int metric, int order, bool f16, const RefineBatch &a, hipStream_t s)
{
    if (a.nq <= 0 || a.nq > 65535 || a.c <= 0) return;
    if (f16) launch_refine_scan_t<_Float16>(metric, order, a, s);
    else launch_refine_scan_t<float>(metric, order, a, s);
}

} // namespace lb
