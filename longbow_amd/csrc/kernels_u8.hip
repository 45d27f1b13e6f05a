// kernels_u8.hip -- the uint8 index (lb_gpu_index_new_u8): exact scan, generic scan, sampled threshold, query widening.
//
// The arithmetic is the reference's one DataTypeUint8 registry kernel, euclideanUint8Unrolled4x (lb_u8_exact.h spells it out):
// four f32 chains, ((s0 + s1) + s2) + s3, sqrt in f64 rounded to f32.  All its partial sums are integers <= S = sum (x_i - q_i)^2,
// so for S <= 2^24 the value is sqrt_rn(float(S)), and S is cheap and exact in integers: |x|^2 + |q|^2 - 2 x.q, with x.q AND
// |x|^2 from v_dot4_u32_u8 in one loop over the staged row (no stored row norms: the index keeps no side array for its rows,
// the second dot costs one instruction per 4 bytes of a row that is in registers anyway, and Add and Compact have nothing to
// recompute).  A pair with S > 2^24 is first tested against the query's threshold by a lower bound of its value
// (u8_value_lower_bound); only a pair that could still be admitted is recomputed, by the lane itself, by the chain arithmetic
// straight from memory.  For D <= 258 no pair leaves the integer path (258 * 65025 < 2^24).
//
// Every lane computes the exact value of its (row, query) pairs, so the candidate entries ARE the results: the lists, the
// sampled threshold, the selects and the emit of the scan path (index_search.hip: run_scan_path) work on them unchanged.
// The kernels read the queries widened to f32 (exact: they are uint8 values) and narrow them back as they stage them.
#include "lb_device.h"
#include "lb_u8_exact.h"

#pragma clang fp contract(off)

namespace lb {

struct ScanU8Args {
    const uint8_t *X;
    int64_t row_begin, row_end;
    int D;
    const float *Q;
    const int *qsel;
    int nsel;
    const uint8_t *mask;
    const uint32_t *rowmap;
    CandState cs;
    int boot;
    int striped;
};

// admission of one finished (position, slot) entry: the f32 scan's rules (kernels_scan.hip: scan_kernel)
__device__ __forceinline__ void u8_admit(const ScanU8Args &a, int j, int qj, uint64_t tau, int64_t pos, uint64_t ent)
{
    if (a.boot) {
        a.cs.lists[(size_t)qj * a.cs.cap + (pos - a.row_begin)] = ent;
    } else if (ent < tau) {
        uint32_t p;
        if (a.striped) {
            const uint32_t st = blockIdx.x & (LB_STRIPES - 1);
            p = st + LB_STRIPES * atomicAdd(&a.cs.stripes[(j * LB_STRIPES + st) * LB_STRIPE_PAD], 1u);
        } else {
            p = atomicAdd(&a.cs.cnt[qj], 1u);
        }
        if (p < a.cs.cap) a.cs.lists[(size_t)qj * a.cs.cap + p] = ent;
    }
}

// the entry of a pair whose exact sum is S, or kEntryMax for a pair that cannot be admitted below tau.  S <= 2^24: the value
// from S.  Beyond: dropped if already the lower bound of its value is no entry below tau (a boot pass keeps every row, so it
// has no such test), else the chains from memory.
__device__ __forceinline__ uint64_t u8_entry(uint32_t S, const uint8_t *x, const float *q, int D, uint32_t row, uint64_t tau, bool boot)
{
    if (S <= U8_EXACT_S) return pack_entry(u8_value_of_s(S), row);
    if (!boot && pack_entry(u8_value_lower_bound(S, D), row) >= tau) return kEntryMax;
    return pack_entry((float)sqrt((double)u8_chain_sum<true>(x, q, D)), row);
}

// ---- staged scan: D % 16 == 0, 16-B aligned rows ------------------------------------------------------------------------
// One lane per row, 256 rows per tile, up to 8 query slots per corpus pass.  A stage is 64 bytes of each of the tile's rows,
// loaded as four coalesced 16-B pieces per thread into an LDS tile with an 80-B row stride (a wave's ds_read_b128 by rows
// then touch every bank equally often), plus the slots' 64 bytes narrowed from f32, which every lane reads at the same
// address (a broadcast).  The next stage's pieces are in flight while the current one is consumed.
constexpr int U8_ROWS = 256;
constexpr int U8_CK = 64;         // bytes per row per stage
constexpr int U8_LD = U8_CK + 16; // LDS row stride (bytes)

__device__ __forceinline__ uint32_t pack_u8x4(float a, float b, float c, float d)
{
    return (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16) | ((uint32_t)d << 24);
}

template <int NQ, bool MAPPED>
__global__ __launch_bounds__(U8_ROWS) void scan_u8_kernel(ScanU8Args a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lx[U8_ROWS * U8_LD];
    __shared__ __attribute__((aligned(16))) uint32_t lq[NQ * U8_CK / 4];
    __shared__ uint32_t qn[NQ];
    const int tid = threadIdx.x;
    const int D = a.D;
    const int nchunks = (D + U8_CK - 1) / U8_CK;
    const int64_t nrows = a.row_end - a.row_begin;
    const int64_t ntiles = (nrows + U8_ROWS - 1) / U8_ROWS;
    if ((int64_t)blockIdx.x >= ntiles) return;

    int qidx[NQ];
    uint64_t tau[NQ];
#pragma unroll
    for (int j = 0; j < NQ; j++) {
        const int jj = j < a.nsel ? j : a.nsel - 1;
        qidx[j] = __builtin_amdgcn_readfirstlane(a.qsel ? a.qsel[jj] : jj);
        tau[j] = j < a.nsel ? a.cs.tau[qidx[j]] : 0ull;
    }
    // the slots' exact |q|^2, once per workgroup (<= 8192 * 255^2 < 2^30)
    if (tid < NQ) qn[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NQ; j++) {
        const float *q = a.Q + (int64_t)qidx[j] * D;
        uint32_t s = 0;
        for (int i = tid; i < D; i += U8_ROWS) {
            const uint32_t v = (uint32_t)q[i];
            s += v * v;
        }
        atomicAdd(&qn[j], s);
    }
    __syncthreads();

    const bool q_loader = tid < NQ * (U8_CK / 4);
    const float *q_src = a.Q + (int64_t)qidx[q_loader ? tid / (U8_CK / 4) : 0] * D;
    u32x4 stg[4];
    uint32_t stq = 0;
    uint32_t rid[MAPPED ? 4 : 1];
    auto load_stage = [&](int64_t tile, int c) {
        const int64_t trow0 = a.row_begin + tile * U8_ROWS;
        const int d0 = c * U8_CK;
        if (q_loader) {
            const int k = d0 + (tid & (U8_CK / 4 - 1)) * 4;
            stq = 0;
            if (k < D) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(q_src + k);
                stq = pack_u8x4(v.x, v.y, v.z, v.w);
            }
        }
        if (MAPPED && c == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int64_t pos = trow0 + ((tid + U8_ROWS * i) >> 2);
                if (pos >= a.row_end) pos = a.row_end - 1;
                rid[MAPPED ? i : 0] = a.rowmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int ch = tid + U8_ROWS * i;
            const int r = ch >> 2, p = ch & 3;
            int64_t row = trow0 + r;
            if (row >= a.row_end) row = a.row_end - 1; // (a partial tile reads its last row again: inside the corpus)
            if (MAPPED) row = rid[MAPPED ? i : 0];
            const int k = d0 + p * 16;
            stg[i] = u32x4{0, 0, 0, 0};
            if (k < D) stg[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(a.X + row * (int64_t)D + k)); // streamed once
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int ch = tid + U8_ROWS * i;
            *reinterpret_cast<u32x4 *>(&lx[(ch >> 2) * U8_LD + (ch & 3) * 16]) = stg[i];
        }
        if (q_loader) lq[tid] = stq;
    };

    uint32_t acc[NQ], xn = 0;
    int64_t tile = blockIdx.x;
    int c = 0;
    load_stage(tile, 0);
    write_stage();
    __syncthreads();
    while (true) {
        int64_t ntile = tile;
        int nc = c + 1;
        if (nc == nchunks) {
            nc = 0;
            ntile = tile + gridDim.x;
        }
        const bool has_next = ntile < ntiles;
        if (has_next) load_stage(ntile, nc);
        if (c == 0) {
            xn = 0;
#pragma unroll
            for (int j = 0; j < NQ; j++) acc[j] = 0;
        }
        {
            const u32x4 *xr = reinterpret_cast<const u32x4 *>(&lx[tid * U8_LD]);
            const u32x4 xv[4] = {xr[0], xr[1], xr[2], xr[3]};
#pragma unroll
            for (int v = 0; v < 4; v++) { // |x|^2 of the piece (bytes beyond D are zero)
                xn = __builtin_amdgcn_udot4(xv[v].x, xv[v].x, xn, false);
                xn = __builtin_amdgcn_udot4(xv[v].y, xv[v].y, xn, false);
                xn = __builtin_amdgcn_udot4(xv[v].z, xv[v].z, xn, false);
                xn = __builtin_amdgcn_udot4(xv[v].w, xv[v].w, xn, false);
            }
#pragma unroll
            for (int j = 0; j < NQ; j++) {
                const u32x4 *qr = reinterpret_cast<const u32x4 *>(&lq[j * (U8_CK / 4)]);
                uint32_t s = acc[j];
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const u32x4 qv = qr[v];
                    s = __builtin_amdgcn_udot4(xv[v].x, qv.x, s, false);
                    s = __builtin_amdgcn_udot4(xv[v].y, qv.y, s, false);
                    s = __builtin_amdgcn_udot4(xv[v].z, qv.z, s, false);
                    s = __builtin_amdgcn_udot4(xv[v].w, qv.w, s, false);
                }
                acc[j] = s;
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (c == nchunks - 1) { // the tile's sums are complete: values and admission
            const int64_t pos = a.row_begin + tile * U8_ROWS + tid;
            if (pos < a.row_end) {
                const int64_t row = MAPPED ? (int64_t)a.rowmap[pos] : pos;
                const bool hidden = a.mask != nullptr && !a.mask[row];
#pragma unroll
                for (int j = 0; j < NQ; j++) {
                    if (j >= a.nsel) break;
                    if (hidden) {
                        if (a.boot) u8_admit(a, j, qidx[j], tau[j], pos, kEntryMax);
                        continue;
                    }
                    const uint32_t S = xn + qn[j] - 2u * acc[j]; // exact: sum (x_i - q_i)^2 < 2^30
                    const uint64_t ent = u8_entry(S, a.X + row * (int64_t)D, a.Q + (int64_t)qidx[j] * D, D, (uint32_t)row, tau[j], a.boot != 0);
                    if (ent == kEntryMax && !a.boot) continue;
                    u8_admit(a, j, qidx[j], tau[j], pos, ent);
                }
            }
        }
        if (has_next) write_stage();
        __syncthreads();
        if (!has_next) break;
        tile = ntile;
        c = nc;
    }
}

// ---- any other D, or a misaligned base: one lane per row, the chain arithmetic throughout -------------------------------
__global__ __launch_bounds__(256) void scan_u8_generic_kernel(ScanU8Args a)
{
    const int D = a.D;
    for (int64_t pos = a.row_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < a.row_end;
         pos += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = a.rowmap ? (int64_t)a.rowmap[pos] : pos;
        const bool hidden = a.mask != nullptr && !a.mask[row];
        for (int j = 0; j < a.nsel; j++) {
            const int qj = a.qsel ? a.qsel[j] : j;
            if (hidden) {
                if (a.boot) a.cs.lists[(size_t)qj * a.cs.cap + (pos - a.row_begin)] = kEntryMax;
                continue;
            }
            const float dist = u8_pair_distance(a.X + row * (int64_t)D, a.Q + (int64_t)qj * D, D);
            u8_admit(a, j, qj, a.cs.tau[qj], pos, pack_entry(dist, (uint32_t)row));
        }
    }
}

bool scan_u8_staged(int D, const void *X) { return D % 16 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0; }

template <int NQ>
static void launch_scan_u8_nq(bool mapped, dim3 grid, hipStream_t s, const ScanU8Args &a)
{
    if (mapped) hipLaunchKernelGGL((scan_u8_kernel<NQ, true>), grid, dim3(U8_ROWS), 0, s, a);
    else hipLaunchKernelGGL((scan_u8_kernel<NQ, false>), grid, dim3(U8_ROWS), 0, s, a);
}

void launch_scan_u8(const uint8_t *X, int64_t row_begin, int64_t row_end, int D, const float *Q, const int *qsel, int nsel,
                    const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool boot, hipStream_t s, bool striped)
{
    if (row_end <= row_begin || nsel <= 0) return;
    ScanU8Args a;
    a.X = X; a.row_begin = row_begin; a.row_end = row_end; a.D = D;
    a.Q = Q; a.qsel = qsel; a.nsel = nsel; a.mask = mask; a.rowmap = rowmap; a.cs = cs;
    a.boot = boot ? 1 : 0;
    a.striped = (striped && cs.stripes != nullptr && !boot) ? 1 : 0;
    if (!scan_u8_staged(D, X)) {
        int64_t blocks = (row_end - row_begin + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(scan_u8_generic_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
        return;
    }
    const int64_t ntiles = (row_end - row_begin + U8_ROWS - 1) / U8_ROWS;
    const int64_t maxgrid = 256 * 8; // 21 KB of LDS and 4 waves a workgroup: 8 workgroups on each of the 256 CUs
    const dim3 grid((unsigned)(ntiles < maxgrid ? ntiles : maxgrid));
    if (nsel <= 1) launch_scan_u8_nq<1>(rowmap != nullptr, grid, s, a);
    else if (nsel <= 2) launch_scan_u8_nq<2>(rowmap != nullptr, grid, s, a);
    else if (nsel <= 4) launch_scan_u8_nq<4>(rowmap != nullptr, grid, s, a);
    else launch_scan_u8_nq<8>(rowmap != nullptr, grid, s, a);
}

// ---- sampled threshold: exact values of `count` evenly spaced positions of [0, span) ---------------------------------
// (as sample_scores_kernel: lists[q][i] = the i-th sample's entry, hidden rows kEntryMax; the first workgroup clears the
// slots' flags).  One lane per (sample, slot), the chain arithmetic.
__global__ __launch_bounds__(256) void sample_u8_kernel(const uint8_t *X, int D, int64_t span, uint32_t count, const uint32_t *rowmap,
                                                        const uint8_t *mask, const float *Q, const int *qsel, int nsel, CandState cs)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (uint64_t)nsel) cs.flags[qsel ? qsel[t] : (int)t] = 0;
    if (t >= (uint64_t)count * (uint64_t)nsel) return;
    const uint32_t i = (uint32_t)(t / (uint64_t)nsel);
    const int j = (int)(t % (uint64_t)nsel);
    const int qj = qsel ? qsel[j] : j;
    const int64_t pos = (int64_t)(((uint64_t)i * (uint64_t)span) / count);
    const int64_t row = rowmap ? (int64_t)rowmap[pos] : pos;
    uint64_t ent = kEntryMax;
    if (mask == nullptr || mask[row]) ent = pack_entry(u8_pair_distance(X + row * (int64_t)D, Q + (int64_t)qj * D, D), (uint32_t)row);
    cs.lists[(size_t)qj * cs.cap + i] = ent;
}

void launch_sample_scores_u8(const uint8_t *X, int D, int64_t span, uint32_t count, const uint32_t *rowmap, const uint8_t *mask,
                             const float *Q, const int *qsel, int nsel, CandState cs, hipStream_t s)
{
    if (count == 0 || nsel <= 0) return;
    const uint64_t threads = (uint64_t)count * (uint64_t)nsel;
    hipLaunchKernelGGL(sample_u8_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, X, D, span, count, rowmap, mask, Q, qsel,
                       nsel, cs);
}

// ---- uint8 queries widened to f32 (exact) -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void widen_u8_kernel(const uint8_t *src, float *dst, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (float)src[i];
}
void launch_widen_u8(const void *src, float *dst, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(widen_u8_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s,
                       static_cast<const uint8_t *>(src), dst, n);
}

} // namespace lb
