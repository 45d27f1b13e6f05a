// kernels_i8.hip -- the int8 index (lb_gpu_index_new_i8): exact scan, i8 MFMA pass, sampled threshold, row and query norms.
//
// The arithmetic is the reference's DataTypeInt8 registry kernels (internal/simd/dispatch.go:241-242):
//   L2   euclideanInt8AVX2Kernel (simd_amd64.s:734-812): with m = 16 floor(D / 16), the main sum of (a_i - b_i)^2 over i < m
//        in exact int32 (<= 8192 * 65025 < 2^31), converted once to f32 (round to nearest), then the tail elements
//        i in [m, D) added in f32 one by one, in order, then sqrt correctly rounded;
//   dot  dotInt8Unrolled4x (simd_baseline.go:37-54): four f32 chains over the residues i mod 4, the tail in chain 0, total
//        ((p0 + p1) + p2) + p3.  The index refuses a dimension with floor(D / 4) + D mod 4 > 1024, so every chain is an exact
//        integer below 2^24 and only the three chain sums round; for D <= 1024 the value is the integer sum itself.
// Reported: L2 the value, dot its negation (ascending lists), exactly as the f32 index reports its own metrics.
//
// Every lane computes the exact value of its (row, query) pairs, so the candidate entries ARE the results: the lists, the
// sampled threshold, the selects and the emit of the scan path (index_search.hip: run_scan_path) work on them unchanged.
// The scan kernels read the queries widened to f32 (exact: they are int8 values) and narrow them back as they stage them; the
// MFMA pass reads the int8 queries.
#include "lb_device.h"
#include "lb_i8_exact.h"

#pragma clang fp contract(off)

namespace lb {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// (the reference value of one pair, one lane, straight from memory, any D: i8_pair_distance of lb_i8_exact.h)

// ---- admission of one finished (position, slot) value: the f32 scan's rules (kernels_scan.hip: scan_kernel) ---------
struct ScanI8Args {
    const int8_t *X;
    int64_t row_begin, row_end;
    int D;
    const float *Q;
    const int *qsel;
    int nsel;
    const int32_t *norm2; // per row: sum of x_i^2 over i < 16 floor(D / 16), exact (L2)
    const uint8_t *mask;
    const uint32_t *rowmap;
    CandState cs;
    int boot;
    int striped;
};

__device__ __forceinline__ void i8_admit(const ScanI8Args &a, int j, int qj, uint64_t tau, int64_t pos, uint64_t ent)
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

// ---- staged scan: D % 16 == 0 (L2 any such D, dot D <= 1024) ------------------------------------------------------------
// One lane per row, 256 rows per tile.  A stage is 64 bytes of each of the tile's rows, loaded as four coalesced 16-B pieces
// per thread into an LDS tile with an 80-B row stride (conflict-free ds_read_b128 by rows), plus the NQ query slots' 64 bytes
// narrowed from f32.  The next stage's pieces are in flight while the current one is consumed.  x.q by v_dot4c_i32_i8,
// exact; L2 sums come from the exact row and query norms: S = |x|^2 + |q|^2 - 2 x.q.
constexpr int I8_ROWS = 256;
constexpr int I8_CK = 64;            // bytes per row per stage
constexpr int I8_LD = I8_CK + 16;    // LDS row stride (bytes)

__device__ __forceinline__ int pack_i8x4(float a, float b, float c, float d)
{
    return ((int)a & 255) | (((int)b & 255) << 8) | (((int)c & 255) << 16) | ((int)d << 24);
}

template <int METRIC, int NQ, bool MAPPED>
__global__ __launch_bounds__(I8_ROWS) void scan_i8_kernel(ScanI8Args a)
{
    __shared__ __attribute__((aligned(16))) int8_t lx[I8_ROWS * I8_LD];
    __shared__ __attribute__((aligned(16))) int lq[NQ * I8_CK / 4];
    __shared__ int qn[NQ];
    const int tid = threadIdx.x;
    const int D = a.D;
    const int nchunks = (D + I8_CK - 1) / I8_CK;
    const int64_t nrows = a.row_end - a.row_begin;
    const int64_t ntiles = (nrows + I8_ROWS - 1) / I8_ROWS;
    if ((int64_t)blockIdx.x >= ntiles) return;

    int qidx[NQ];
    uint64_t tau[NQ];
#pragma unroll
    for (int j = 0; j < NQ; j++) {
        const int jj = j < a.nsel ? j : a.nsel - 1;
        qidx[j] = __builtin_amdgcn_readfirstlane(a.qsel ? a.qsel[jj] : jj);
        tau[j] = j < a.nsel ? a.cs.tau[qidx[j]] : 0ull;
    }
    // the slots' exact |q|^2 (L2), once per workgroup
    if (METRIC == METRIC_L2) {
        if (tid < NQ) qn[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            const float *q = a.Q + (int64_t)qidx[j] * D;
            int s = 0;
            for (int i = tid; i < D; i += I8_ROWS) {
                const int v = (int)q[i];
                s += v * v;
            }
            atomicAdd(&qn[j], s);
        }
        __syncthreads();
    }

    const bool q_loader = tid < NQ * (I8_CK / 4);
    const float *q_src = a.Q + (int64_t)qidx[q_loader ? tid / (I8_CK / 4) : 0] * D;
    i32x4 stg[4];
    int stq = 0;
    uint32_t rid[MAPPED ? 4 : 1];
    auto load_stage = [&](int64_t tile, int c) {
        const int64_t trow0 = a.row_begin + tile * I8_ROWS;
        const int d0 = c * I8_CK;
        if (q_loader) {
            const int k = d0 + (tid & (I8_CK / 4 - 1)) * 4;
            stq = 0;
            if (k < D) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(q_src + k);
                stq = pack_i8x4(v.x, v.y, v.z, v.w);
            }
        }
        if (MAPPED && c == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                int64_t pos = trow0 + ((tid + I8_ROWS * i) >> 2);
                if (pos >= a.row_end) pos = a.row_end - 1;
                rid[MAPPED ? i : 0] = a.rowmap[pos];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int ch = tid + I8_ROWS * i;
            const int r = ch >> 2, p = ch & 3;
            int64_t row = trow0 + r;
            if (row >= a.row_end) row = a.row_end - 1;
            if (MAPPED) row = rid[MAPPED ? i : 0];
            const int k = d0 + p * 16;
            stg[i] = i32x4{0, 0, 0, 0};
            if (k < D) stg[i] = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(a.X + row * (int64_t)D + k)); // streamed once
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int ch = tid + I8_ROWS * i;
            *reinterpret_cast<i32x4 *>(&lx[(ch >> 2) * I8_LD + (ch & 3) * 16]) = stg[i];
        }
        if (q_loader) lq[tid] = stq;
    };

    int acc[NQ];
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
#pragma unroll
            for (int j = 0; j < NQ; j++) acc[j] = 0;
        }
        {
            const i32x4 *xr = reinterpret_cast<const i32x4 *>(&lx[tid * I8_LD]);
            const i32x4 x0 = xr[0], x1 = xr[1], x2 = xr[2], x3 = xr[3];
#pragma unroll
            for (int j = 0; j < NQ; j++) {
                const i32x4 *qr = reinterpret_cast<const i32x4 *>(&lq[j * (I8_CK / 4)]);
                const i32x4 q0 = qr[0], q1 = qr[1], q2 = qr[2], q3 = qr[3];
                int s = acc[j];
                s = __builtin_amdgcn_sdot4(x0.x, q0.x, s, false);
                s = __builtin_amdgcn_sdot4(x0.y, q0.y, s, false);
                s = __builtin_amdgcn_sdot4(x0.z, q0.z, s, false);
                s = __builtin_amdgcn_sdot4(x0.w, q0.w, s, false);
                s = __builtin_amdgcn_sdot4(x1.x, q1.x, s, false);
                s = __builtin_amdgcn_sdot4(x1.y, q1.y, s, false);
                s = __builtin_amdgcn_sdot4(x1.z, q1.z, s, false);
                s = __builtin_amdgcn_sdot4(x1.w, q1.w, s, false);
                s = __builtin_amdgcn_sdot4(x2.x, q2.x, s, false);
                s = __builtin_amdgcn_sdot4(x2.y, q2.y, s, false);
                s = __builtin_amdgcn_sdot4(x2.z, q2.z, s, false);
                s = __builtin_amdgcn_sdot4(x2.w, q2.w, s, false);
                s = __builtin_amdgcn_sdot4(x3.x, q3.x, s, false);
                s = __builtin_amdgcn_sdot4(x3.y, q3.y, s, false);
                s = __builtin_amdgcn_sdot4(x3.z, q3.z, s, false);
                s = __builtin_amdgcn_sdot4(x3.w, q3.w, s, false);
                acc[j] = s;
            }
        }
        __syncthreads(); // every wave is done reading the stage
        if (c == nchunks - 1) { // the tile's sums are complete: values and admission
            const int64_t pos = a.row_begin + tile * I8_ROWS + tid;
            if (pos < a.row_end) {
                const int64_t row = MAPPED ? (int64_t)a.rowmap[pos] : pos;
                const bool hidden = a.mask != nullptr && !a.mask[row];
                const int xn = METRIC == METRIC_L2 ? a.norm2[row] : 0;
#pragma unroll
                for (int j = 0; j < NQ; j++) {
                    if (j >= a.nsel) break;
                    float dist;
                    if (METRIC == METRIC_L2) dist = (float)sqrt((double)(float)(xn + qn[j] - 2 * acc[j]));
                    else dist = -(float)acc[j]; // |x.q| <= 2^24: exact
                    const uint64_t ent = hidden ? kEntryMax : pack_entry(dist, (uint32_t)row);
                    if (hidden && !a.boot) continue;
                    i8_admit(a, j, qidx[j], tau[j], pos, ent);
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

// ---- any other D (or dot beyond 1024 dimensions): one lane per row, straight from memory ------------------------------
template <int METRIC>
__global__ __launch_bounds__(256) void scan_i8_generic_kernel(ScanI8Args a)
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
            const float dist = i8_pair_distance<METRIC>(a.X + row * (int64_t)D, a.Q + (int64_t)qj * D, D);
            i8_admit(a, j, qj, a.cs.tau[qj], pos, pack_entry(dist, (uint32_t)row));
        }
    }
}

bool scan_i8_staged(int metric, int D, const void *X)
{
    return D % 16 == 0 && (metric == METRIC_L2 || D <= 1024) && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
}

template <int METRIC, int NQ>
static void launch_scan_i8_nq(bool mapped, dim3 grid, hipStream_t s, const ScanI8Args &a)
{
    if (mapped) hipLaunchKernelGGL((scan_i8_kernel<METRIC, NQ, true>), grid, dim3(I8_ROWS), 0, s, a);
    else hipLaunchKernelGGL((scan_i8_kernel<METRIC, NQ, false>), grid, dim3(I8_ROWS), 0, s, a);
}

template <int METRIC>
static void launch_scan_i8_metric(int nsel, bool mapped, dim3 grid, hipStream_t s, const ScanI8Args &a)
{
    if (nsel <= 1) launch_scan_i8_nq<METRIC, 1>(mapped, grid, s, a);
    else if (nsel <= 2) launch_scan_i8_nq<METRIC, 2>(mapped, grid, s, a);
    else if (nsel <= 4) launch_scan_i8_nq<METRIC, 4>(mapped, grid, s, a);
    else launch_scan_i8_nq<METRIC, 8>(mapped, grid, s, a);
}

void launch_scan_i8(int metric, const int8_t *X, int64_t row_begin, int64_t row_end, int D, const float *Q, const int *qsel,
                    int nsel, const int32_t *norm2, const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool boot,
                    hipStream_t s, bool striped)
{
    if (row_end <= row_begin || nsel <= 0) return;
    ScanI8Args a;
    a.X = X; a.row_begin = row_begin; a.row_end = row_end; a.D = D;
    a.Q = Q; a.qsel = qsel; a.nsel = nsel; a.norm2 = norm2; a.mask = mask; a.rowmap = rowmap; a.cs = cs;
    a.boot = boot ? 1 : 0;
    a.striped = (striped && cs.stripes != nullptr && !boot) ? 1 : 0;
    if (!scan_i8_staged(metric, D, X)) {
        int64_t blocks = (row_end - row_begin + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        if (metric == METRIC_L2) hipLaunchKernelGGL((scan_i8_generic_kernel<METRIC_L2>), dim3((unsigned)blocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((scan_i8_generic_kernel<METRIC_DOT>), dim3((unsigned)blocks), dim3(256), 0, s, a);
        return;
    }
    const int64_t ntiles = (row_end - row_begin + I8_ROWS - 1) / I8_ROWS;
    const int64_t maxgrid = 256 * 8; // 21 KB of LDS and 4 waves a workgroup: 8 workgroups on each of the 256 CUs
    const dim3 grid((unsigned)(ntiles < maxgrid ? ntiles : maxgrid));
    if (metric == METRIC_L2) launch_scan_i8_metric<METRIC_L2>(nsel, rowmap != nullptr, grid, s, a);
    else launch_scan_i8_metric<METRIC_DOT>(nsel, rowmap != nullptr, grid, s, a);
}

// ---- sampled threshold: exact values of `count` evenly spaced positions of [0, span) ---------------------------------
// (as sample_scores_kernel: lists[q][i] = the i-th sample's entry, hidden rows kEntryMax; the first workgroup clears the
// slots' flags).  One lane per (sample, slot).
template <int METRIC>
__global__ __launch_bounds__(256) void sample_i8_kernel(const int8_t *X, int D, int64_t span, uint32_t count, const uint32_t *rowmap,
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
    if (mask == nullptr || mask[row]) ent = pack_entry(i8_pair_distance<METRIC>(X + row * (int64_t)D, Q + (int64_t)qj * D, D), (uint32_t)row);
    cs.lists[(size_t)qj * cs.cap + i] = ent;
}

void launch_sample_scores_i8(int metric, const int8_t *X, int D, int64_t span, uint32_t count, const uint32_t *rowmap,
                             const uint8_t *mask, const float *Q, const int *qsel, int nsel, CandState cs, hipStream_t s)
{
    if (count == 0 || nsel <= 0) return;
    const uint64_t threads = (uint64_t)count * (uint64_t)nsel;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (metric == METRIC_L2) hipLaunchKernelGGL((sample_i8_kernel<METRIC_L2>), grid, dim3(256), 0, s, X, D, span, count, rowmap, mask, Q, qsel, nsel, cs);
    else hipLaunchKernelGGL((sample_i8_kernel<METRIC_DOT>), grid, dim3(256), 0, s, X, D, span, count, rowmap, mask, Q, qsel, nsel, cs);
}

// ---- side data at Add time: per row the exact sum of x_i^2 over i < 16 floor(D / 16), one wave per row ----------------
__global__ __launch_bounds__(256) void row_norms_i8_kernel(const int8_t *X, int64_t n, int D, int32_t *norm2)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int m = D & ~15;
    const int8_t *x = X + row * (int64_t)D;
    int s = 0;
    for (int i = lane; i < m; i += 64) s += (int)x[i] * (int)x[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) norm2[row] = s;
}

void launch_row_norms_i8(const int8_t *X, int64_t n, int D, int32_t *norm2, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(row_norms_i8_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, X, n, D, norm2);
}

// ---- i8 MFMA pass: batches of queries, D % 16 == 0 (L2 any such D, dot D <= 1024) -----------------------------------------
// A workgroup holds 128 query slots (blockIdx.y) and walks tiles of 128 positions; its four waves own 64 x 64 quarters of the
// 128 x 128 output, as 2 x 2 blocks of v_mfma_i32_32x32x32_i8 (A = rows, B = queries; x.q exact in int32).  A stage is 128
// bytes of each row and query, 16-B pieces into LDS (144-B row stride), zero beyond D: the MFMA's K of 32 is padded there.
// The (tile, stage) sequence is one flat pipeline: the next stage's pieces are loaded into registers while the current stage
// feeds the matrix cores.
// Operand fragments: lane l (r = l & 31, h = l >> 5) takes the 16 bytes [32 s + 16 h, +16) of row / query r for the k-step s,
// A and B alike, so whatever order the instruction gives the 16 bytes of a lane, it pairs equal k.  Outputs: query column
// l & 31, row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) of the block (the gfx950 C/D map).
// Each output's key is the exact integer S (L2 |x|^2 + |q|^2 - 2 x.q, dot -x.q) and from it the exact value: L2 the monotone
// sqrt_rn(float_rn(S)) (D % 16 == 0: no tail), dot float(S) (exact below 2^24).  So the entries are the scan's:
// sample = 1: positions are the `count` sampled positions of [0, span); every entry goes to lists[q][position] (the sampled
//             threshold's input, as launch_sample_scores writes it);
// sample = 0: positions are the row view's; an entry below tau[q] is admitted to q's list (L2: a row whose S is beyond the
//             integer bound smax(tau) >= S of any admissible entry skips the conversion).
constexpr int MF_ROWS = 128, MF_QS = 128, MF_CK = 128, MF_LD = MF_CK + 16;
constexpr int MF_PPR = MF_CK / 16; // 16-B pieces per row per stage
constexpr int MF_PT = MF_ROWS * MF_PPR / 256; // pieces per thread per stage (rows; the queries alike)
typedef int i32x16 __attribute__((ext_vector_type(16)));

struct MfmaI8Args {
    const int8_t *X;
    int64_t npos; // positions walked: the row view's (rowmap / all rows), or `count` samples
    int D;
    const int8_t *Q8; // nq int8 queries, row-major, 16-B aligned rows
    int nq;
    const int32_t *qn;    // [nq] exact |q|^2 (launch_query_norms_i8)
    const int32_t *norm2; // per row (launch_row_norms_i8)
    const uint8_t *mask;
    const uint32_t *rowmap;
    CandState cs;
    int sample;
    int64_t span;
};

// corpus row behind position pos of the walk (clamped into it)
__device__ __forceinline__ uint32_t mf_row(const MfmaI8Args &a, int64_t pos)
{
    if (pos >= a.npos) pos = a.npos - 1;
    const int64_t vpos = a.sample ? (int64_t)(((uint64_t)pos * (uint64_t)a.span) / (uint64_t)a.npos) : pos;
    return a.rowmap ? a.rowmap[vpos] : (uint32_t)vpos;
}

// (launch bounds: three waves per SIMD -- 168 registers, 4 of them spilled in the L2 form; at the ~240 the compiler picks
// unbounded only two workgroups fit a CU and 1024 queries over 1M x 768 took 3.3 ms instead of 2.6)
template <int METRIC>
__global__ __launch_bounds__(256, 3) void mfma_i8_kernel(MfmaI8Args a)
{
    __shared__ __attribute__((aligned(16))) int8_t lx[MF_ROWS * MF_LD];
    __shared__ __attribute__((aligned(16))) int8_t lq[MF_QS * MF_LD];
    __shared__ uint32_t lrow[2][MF_ROWS]; // per parity of the tiles walked: corpus row, |x|^2, (2: past the walk | 1: masked out)
    __shared__ int lnx[2][MF_ROWS];
    __shared__ uint8_t lhid[2][MF_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave & 1, wq = wave >> 1;
    const int D = a.D;
    const int nchunks = (D + MF_CK - 1) / MF_CK;
    const int64_t ntiles = (a.npos + MF_ROWS - 1) / MF_ROWS;
    if ((int64_t)blockIdx.x >= ntiles) return;
    const int q0 = blockIdx.y * MF_QS;

    // this lane's two query columns q0 + wq * 64 + bj * 32 + (lane & 31): threshold, integer bound, norm
    uint64_t tau[2];
    int smax[2], qnl[2];
#pragma unroll
    for (int bj = 0; bj < 2; bj++) {
        const int q = q0 + wq * 64 + bj * 32 + (lane & 31);
        const int qc = q < a.nq ? q : a.nq - 1;
        tau[bj] = a.sample ? kEntryMax : a.cs.tau[qc];
        qnl[bj] = METRIC == METRIC_L2 ? a.qn[qc] : 0;
        smax[bj] = 0x7fffffff;
        if (METRIC == METRIC_L2 && tau[bj] != kEntryMax) {
            const double tk = (double)entry_key(tau[bj]);
            const double b = tk * tk * (1.0 + 0x1p-20);
            if (b < 2147483647.0) smax[bj] = (int)b; // S > smax => value > tau's key
        }
    }

    uint32_t rid[MF_PT];
    i32x4 px[MF_PT], pq[MF_PT];
    auto tile_rows = [&](int64_t t) { // this thread's staging rows of tile t, and (tid < 128) its metadata
#pragma unroll
        for (int i = 0; i < MF_PT; i++) rid[i] = mf_row(a, t * MF_ROWS + ((tid + 256 * i) / MF_PPR));
    };
    auto tile_meta = [&](int64_t t, int p) {
        if (tid < MF_ROWS) {
            const int64_t pos = t * MF_ROWS + tid;
            const uint32_t row = mf_row(a, pos);
            lrow[p][tid] = row;
            lnx[p][tid] = METRIC == METRIC_L2 ? a.norm2[row] : 0;
            lhid[p][tid] = (pos >= a.npos ? 2 : 0) | ((a.mask != nullptr && !a.mask[row]) ? 1 : 0);
        }
    };
    auto load_stage = [&](int c) {
        const int d0 = c * MF_CK;
#pragma unroll
        for (int i = 0; i < MF_PT; i++) {
            const int ch = tid + 256 * i;
            const int r = ch / MF_PPR, k = d0 + (ch % MF_PPR) * 16;
            px[i] = i32x4{0, 0, 0, 0};
            pq[i] = i32x4{0, 0, 0, 0};
            if (k < D) {
                px[i] = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(a.X + (int64_t)rid[i] * D + k)); // streamed once
                const int q = q0 + r;
                if (q < a.nq) pq[i] = *reinterpret_cast<const i32x4 *>(a.Q8 + (int64_t)q * D + k);
            }
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < MF_PT; i++) {
            const int ch = tid + 256 * i;
            const int o = (ch / MF_PPR) * MF_LD + (ch % MF_PPR) * 16;
            *reinterpret_cast<i32x4 *>(&lx[o]) = px[i];
            *reinterpret_cast<i32x4 *>(&lq[o]) = pq[i];
        }
    };

    i32x16 acc[2][2];
    int64_t tile = blockIdx.x;
    int c = 0, par = 0; // par: parity of the tiles this workgroup has walked (not of the tile index: gridDim.x may be even)
    tile_rows(tile);
    tile_meta(tile, 0);
    load_stage(0);
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
        if (has_next) {
            if (nc == 0) tile_rows(ntile);
            load_stage(nc);
        }
        if (c == 0) {
#pragma unroll
            for (int bi = 0; bi < 2; bi++)
#pragma unroll
                for (int bj = 0; bj < 2; bj++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[bi][bj][e] = 0;
        }
#pragma unroll
        for (int st = 0; st < MF_CK / 32; st++) {
            const int off = st * 32 + (lane >> 5) * 16;
            i32x4 fa[2], fb[2];
#pragma unroll
            for (int b = 0; b < 2; b++) {
                fa[b] = *reinterpret_cast<const i32x4 *>(&lx[(wr * 64 + b * 32 + (lane & 31)) * MF_LD + off]);
                fb[b] = *reinterpret_cast<const i32x4 *>(&lq[(wq * 64 + b * 32 + (lane & 31)) * MF_LD + off]);
            }
#pragma unroll
            for (int bi = 0; bi < 2; bi++)
#pragma unroll
                for (int bj = 0; bj < 2; bj++)
                    acc[bi][bj] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[bi], fb[bj], acc[bi][bj], 0, 0, 0);
        }
        __syncthreads(); // every wave is done with the stage
        if (has_next) {
            write_stage();
            if (nc == 0) tile_meta(ntile, par ^ 1); // (the other parity: the previous tile's epilogue is behind the barrier above)
        }
        __syncthreads();
        if (c == nchunks - 1) { // epilogue: exact entries, admission
#pragma unroll
            for (int bi = 0; bi < 2; bi++) {
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int rl = wr * 64 + bi * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    const int hid = lhid[par][rl];
                    if (hid & 2) continue;
                    const uint32_t row = lrow[par][rl];
                    const int xn = lnx[par][rl];
                    const int64_t pos = tile * MF_ROWS + rl;
#pragma unroll
                    for (int bj = 0; bj < 2; bj++) {
                        const int q = q0 + wq * 64 + bj * 32 + (lane & 31);
                        if (q >= a.nq) continue;
                        const int dot = acc[bi][bj][e];
                        if (a.sample) {
                            float dist;
                            if (METRIC == METRIC_L2) dist = (float)sqrt((double)(float)(xn + qnl[bj] - 2 * dot));
                            else dist = -(float)dot;
                            a.cs.lists[(size_t)q * a.cs.cap + pos] = hid ? kEntryMax : pack_entry(dist, row);
                            continue;
                        }
                        if (hid) continue;
                        float dist;
                        if (METRIC == METRIC_L2) {
                            const int S = xn + qnl[bj] - 2 * dot;
                            if (S > smax[bj]) continue;
                            dist = (float)sqrt((double)(float)S);
                        } else {
                            dist = -(float)dot;
                        }
                        const uint64_t ent = pack_entry(dist, row);
                        if (ent < tau[bj]) {
                            const uint32_t p = atomicAdd(&a.cs.cnt[q], 1u);
                            if (p < a.cs.cap) a.cs.lists[(size_t)q * a.cs.cap + p] = ent;
                        }
                    }
                }
            }
        }
        if (!has_next) break;
        if (nc == 0) par ^= 1;
        tile = ntile;
        c = nc;
    }
}

bool mfma_i8_supported(int metric, int D, const void *X, const void *Q8)
{
    return D % 16 == 0 && (metric == METRIC_L2 || D <= 1024) && (reinterpret_cast<uintptr_t>(X) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(Q8) & 15) == 0;
}

void launch_mfma_i8(int metric, const int8_t *X, int64_t npos, int D, const int8_t *Q8, int nq, const int32_t *qn,
                    const int32_t *norm2, const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool sample, int64_t span,
                    hipStream_t s)
{
    if (npos <= 0 || nq <= 0) return;
    MfmaI8Args a;
    a.X = X; a.npos = npos; a.D = D; a.Q8 = Q8; a.nq = nq; a.qn = qn; a.norm2 = norm2; a.mask = mask; a.rowmap = rowmap;
    a.cs = cs; a.sample = sample ? 1 : 0; a.span = span;
    const int64_t ntiles = (npos + MF_ROWS - 1) / MF_ROWS;
    const int qtiles = (nq + MF_QS - 1) / MF_QS;
    // the workgroups that fit at once (168 registers a lane, __launch_bounds__: 3 per CU, 256 CUs) over the batch's query tiles;
    // each walks row tiles grid-strided
    int64_t gx = (768 + qtiles - 1) / qtiles;
    if (gx > ntiles) gx = ntiles;
    const dim3 grid((unsigned)gx, (unsigned)qtiles);
    if (metric == METRIC_L2) hipLaunchKernelGGL((mfma_i8_kernel<METRIC_L2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((mfma_i8_kernel<METRIC_DOT>), grid, dim3(256), 0, s, a);
}

// exact |q|^2 of each int8 query, one wave per query
__global__ __launch_bounds__(64) void query_norms_i8_kernel(const int8_t *Q8, int D, int32_t *qn)
{
    const int8_t *q = Q8 + (int64_t)blockIdx.x * D;
    int s = 0;
    for (int i = threadIdx.x; i < D; i += 64) s += (int)q[i] * (int)q[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) qn[blockIdx.x] = s;
}
void launch_query_norms_i8(const int8_t *Q8, int nq, int D, int32_t *qn, hipStream_t s)
{
    if (nq > 0) hipLaunchKernelGGL(query_norms_i8_kernel, dim3((unsigned)nq), dim3(64), 0, s, Q8, D, qn);
}

// ---- int8 queries widened to f32 (exact) ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void widen_i8_kernel(const int8_t *src, float *dst, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (float)src[i];
}
void launch_widen_i8(const void *src, float *dst, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(widen_i8_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s,
                       static_cast<const int8_t *>(src), dst, n);
}

} // namespace lb
