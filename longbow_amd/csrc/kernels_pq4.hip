// kernels_pq4.hip -- 4-bit product quantisation on gfx950: encode + pack, pack / unpack of ready-made codes, and the ADC scan
// over packed rows (lb_pq4.h states the layout).
//
// The scan.  A lane owns a row, a wave owns 64 consecutive rows: one contiguous run of 64 * P bytes.
//   fast form     (P % 16 == 0, 16-byte aligned base, M <= 128) the wave pulls its run into a private LDS slot with P / 16
//                 direct-to-LDS requests of 1 KiB, every lane reads its own row back with ds_read_b128, and the requests of the
//                 wave's NEXT run are issued before the lookups of this one start, so they fly under them.
//   generic form  (any M, any alignment) single bytes, none outside [codes, codes + n * P).
//   lookup        a 16-entry subtable is 16 lanes of one VGPR.  VGPR g of a query holds subtables 4g .. 4g + 3: lane L holds
//                 table[(4g + L / 16) * 16 + L % 16], which is simply table[64 g + L].  Entry (j, c) is one ds_bpermute_b32 of
//                 VGPR j / 4 from lane (j % 4) * 16 + c: the crossbar of the LDS without its memory, no bank conflicts by
//                 construction.  M / 4 VGPRs a query, so up to PQ4_REG_MAX_M subspaces; four queries (two beyond M = 96) share a
//                 pass over the codes, each with its own ordered f32 chain.  ds_bpermute reads 0 from a lane that is switched
//                 off, so every lane of a wave stays on through the lookups and the rows beyond the end are dropped after them.
//                 Beyond PQ4_REG_MAX_M (or when asked: the measurement of DESIGN 3.x) the tables sit in LDS as [M][16] f32 and
//                 a lookup is a ds_read_b32; one or two queries a pass.
//   result        float32(sqrt(float64(s))), s the f32 sum ((0 + t[0][c0]) + t[1][c1]) + ... in j order: no FMA (there is no
//                 product), no reassociation (contraction is off for the file all the same).
#include "lb_pq4.h"
#include "lb_exact.h"

#include <stdexcept>

#pragma clang fp contract(off)

namespace lb {

enum : int { PQ4_REG = 0, PQ4_LDS = 1 };
constexpr int PQ4_THREADS = PQ4_WAVES * 64;
constexpr int PQ4_MAX_BLOCKS = 2048;

// ---------------------------------------------------------------------------------------------------------------------------
// Encode and pack.  One workgroup = 256 vectors x TWO neighbouring subspaces (2p, 2p + 1): their 32 centroids sit in LDS and are
// read as wave-wide broadcasts, a lane keeps its sub-vector in registers and finishes both codes itself, so the packed byte is
// written once.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr float PQ4_FLT_MAX = 3.402823466e+38f;

template <int SUB> __device__ __forceinline__ int pq4_nearest(const float (&v)[SUB], const float *cb)
{
    float bd = PQ4_FLT_MAX;
    int best = 0;
#pragma unroll 2
    for (int k = 0; k < PQ4_K; k++) {
        const float *c = cb + k * SUB;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        constexpr int MAIN = SUB & ~3;
#pragma unroll
        for (int t = 0; t < MAIN; t += 4) {
            const float d0 = v[t] - c[t], d1 = v[t + 1] - c[t + 1], d2 = v[t + 2] - c[t + 2], d3 = v[t + 3] - c[t + 3];
            s0 = s0 + d0 * d0;
            s1 = s1 + d1 * d1;
            s2 = s2 + d2 * d2;
            s3 = s3 + d3 * d3;
        }
#pragma unroll
        for (int t = MAIN; t < SUB; t++) {
            const float d = v[t] - c[t];
            s0 = s0 + d * d;
        }
        float s = s0 + s1;
        s = s + s2;
        s = s + s3;
        if (s < bd) { bd = s; best = k; } // (false for a NaN sum and for +inf: nothing below FLT_MAX leaves code 0)
    }
    return best;
}

// any SubDim: operands straight from global memory
__device__ __forceinline__ int pq4_nearest_any(const float *x, const float *cb, int sub)
{
    const int main4 = sub & ~3;
    float bd = PQ4_FLT_MAX;
    int best = 0;
    for (int k = 0; k < PQ4_K; k++) {
        const float *c = cb + (int64_t)k * sub;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int t = 0; t < main4; t += 4) {
            const float d0 = x[t] - c[t], d1 = x[t + 1] - c[t + 1], d2 = x[t + 2] - c[t + 2], d3 = x[t + 3] - c[t + 3];
            s0 = s0 + d0 * d0;
            s1 = s1 + d1 * d1;
            s2 = s2 + d2 * d2;
            s3 = s3 + d3 * d3;
        }
        for (int t = main4; t < sub; t++) {
            const float d = x[t] - c[t];
            s0 = s0 + d * d;
        }
        float s = s0 + s1;
        s = s + s2;
        s = s + s3;
        if (s < bd) { bd = s; best = k; }
    }
    return best;
}

__device__ __forceinline__ void pq4_store_pair(uint8_t *out, int64_t row, int M, int P, int pr, int c0, int c1, bool two, int packed)
{
    if (packed) {
        out[row * (int64_t)P + pr] = (uint8_t)(c0 | (c1 << 4));
    } else {
        out[row * (int64_t)M + 2 * pr] = (uint8_t)c0;
        if (two) out[row * (int64_t)M + 2 * pr + 1] = (uint8_t)c1;
    }
}

template <int SUB>
__global__ __launch_bounds__(256) void pq4_encode_kernel(const float *codebooks, int M, const float *X, int64_t n, int D, uint8_t *out,
                                                         int packed)
{
    __shared__ __attribute__((aligned(16))) float cb[2 * PQ4_K * SUB];
    const int P = (M + 1) / 2;
    const int pr = blockIdx.x % P;
    const int64_t rb = blockIdx.x / P;
    const bool two = 2 * pr + 1 < M;
    // (subspaces 2p and 2p + 1 lie one after the other in the codebooks)
    const float *src = codebooks + (int64_t)(2 * pr) * PQ4_K * SUB;
    for (int i = threadIdx.x; i < (two ? 2 : 1) * PQ4_K * SUB; i += 256) cb[i] = src[i];
    __syncthreads();
    const int64_t row = rb * 256 + threadIdx.x;
    if (row >= n) return;
    const float *x = X + row * (int64_t)D + (int64_t)(2 * pr) * SUB;
    float v[SUB];
#pragma unroll
    for (int t = 0; t < SUB; t++) v[t] = x[t];
    const int c0 = pq4_nearest<SUB>(v, cb);
    int c1 = 0;
    if (two) {
#pragma unroll
        for (int t = 0; t < SUB; t++) v[t] = x[SUB + t];
        c1 = pq4_nearest<SUB>(v, cb + PQ4_K * SUB);
    }
    pq4_store_pair(out, row, M, P, pr, c0, c1, two, packed);
}

__global__ __launch_bounds__(256) void pq4_encode_any_kernel(const float *codebooks, int M, int sub, const float *X, int64_t n, int D,
                                                             uint8_t *out, int packed)
{
    const int P = (M + 1) / 2;
    const int pr = blockIdx.x % P;
    const int64_t row = (int64_t)(blockIdx.x / P) * 256 + threadIdx.x;
    if (row >= n) return;
    const bool two = 2 * pr + 1 < M;
    const float *x = X + row * (int64_t)D + (int64_t)(2 * pr) * sub;
    const float *cb = codebooks + (int64_t)(2 * pr) * PQ4_K * sub;
    const int c0 = pq4_nearest_any(x, cb, sub);
    const int c1 = two ? pq4_nearest_any(x + sub, cb + (int64_t)PQ4_K * sub, sub) : 0;
    pq4_store_pair(out, row, M, P, pr, c0, c1, two, packed);
}

void launch_pq4_encode(const float *codebooks, int M, int sub, const float *X, int64_t n, uint8_t *out, bool packed, hipStream_t s)
{
    if (n <= 0) return;
    const int D = M * sub, P = pq4_row_bytes(M);
    const int64_t out_row = packed ? P : M;
    // (grid.x carries P x row-blocks with the pair index fastest, so the workgroups that read the same 256 rows run back to back)
    const int64_t rb_total = (n + 255) / 256, max_rb = 0x7fffffffll / P;
    for (int64_t rb0 = 0; rb0 < rb_total; rb0 += max_rb) {
        const int64_t nrb = rb_total - rb0 < max_rb ? rb_total - rb0 : max_rb;
        const int64_t r0 = rb0 * 256, cnt = (n - r0) < nrb * 256 ? (n - r0) : nrb * 256;
        const float *Xs = X + r0 * (int64_t)D;
        uint8_t *os = out + r0 * out_row;
        const dim3 grid((unsigned)(nrb * P)), block(256);
#define LB_ENC4(S) hipLaunchKernelGGL((pq4_encode_kernel<S>), grid, block, 0, s, codebooks, M, Xs, cnt, D, os, packed ? 1 : 0)
        switch (sub) {
        case 1: LB_ENC4(1); break;
        case 2: LB_ENC4(2); break;
        case 4: LB_ENC4(4); break;
        case 8: LB_ENC4(8); break;
        case 12: LB_ENC4(12); break;
        case 16: LB_ENC4(16); break;
        case 32: LB_ENC4(32); break;
        default:
            hipLaunchKernelGGL(pq4_encode_any_kernel, grid, block, 0, s, codebooks, M, sub, Xs, cnt, D, os, packed ? 1 : 0);
            break;
        }
#undef LB_ENC4
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Pack / unpack of ready-made codes: a thread per packed byte / per code.  A byte of 16 or more raises *bad (its low nibble is
// stored: the rows are not committed, pq4.hip reads the flag first).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pq4_pack_kernel(const uint8_t *codes, int M, int P, int64_t n, uint8_t *packed, uint32_t *bad)
{
    const int64_t total = n * (int64_t)P;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / P;
        const int b = (int)(i - row * P);
        const uint32_t lo = codes[row * (int64_t)M + 2 * b];
        const uint32_t hi = 2 * b + 1 < M ? codes[row * (int64_t)M + 2 * b + 1] : 0u;
        if ((lo | hi) >= 16u) *bad = 1u;
        packed[i] = (uint8_t)((lo & 15u) | ((hi & 15u) << 4));
    }
}

__global__ __launch_bounds__(256) void pq4_unpack_kernel(const uint8_t *packed, int M, int P, int64_t n, uint8_t *codes)
{
    const int64_t total = n * (int64_t)M;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / M;
        const int j = (int)(i - row * M);
        const uint32_t byte = packed[row * (int64_t)P + (j >> 1)];
        codes[i] = (uint8_t)((j & 1) ? byte >> 4 : byte & 15u);
    }
}

static unsigned pq4_blocks(int64_t total)
{
    const int64_t b = (total + 255) / 256;
    return (unsigned)(b > 16384 ? 16384 : b);
}

void launch_pq4_pack(const uint8_t *codes, int M, int64_t n, uint8_t *packed, uint32_t *bad, hipStream_t s)
{
    if (n <= 0) return;
    const int P = pq4_row_bytes(M);
    hipLaunchKernelGGL(pq4_pack_kernel, dim3(pq4_blocks(n * P)), dim3(256), 0, s, codes, M, P, n, packed, bad);
}

void launch_pq4_unpack(const uint8_t *packed, int M, int64_t n, uint8_t *codes, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(pq4_unpack_kernel, dim3(pq4_blocks(n * M)), dim3(256), 0, s, packed, M, pq4_row_bytes(M), n, codes);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The row sums: what the scan and the sample kernel score a row through.
// ---------------------------------------------------------------------------------------------------------------------------
// the eight codes of word wi of a row (subspaces 8 wi .. 8 wi + 7, code b in bits [4b, 4b + 4)) onto each query's chain.
// t: the queries' tables in registers (PQ4_REG: wi must be a constant once unrolled); lt: in LDS, m16 floats a query.
// Subspaces below jfree are known to exist; the others are asked against M (a uniform branch): the spare nibble adds nothing.
template <int LOOKUP, int NQ, int NV>
__device__ __forceinline__ void pq4_add_word(float (&sum)[NQ], const float (&t)[NQ][NV], const float *lt, int m16, uint32_t w, int wi, int M,
                                             int jfree)
{
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const int j = wi * 8 + b;
        if (j < jfree || j < M) {
            const uint32_t c = (w >> (4 * b)) & 15u;
            if constexpr (LOOKUP == PQ4_REG) {
                const int addr = (int)(c << 2) + (j & 3) * 64; // byte address of lane (j % 4) * 16 + c
#pragma unroll
                for (int q = 0; q < NQ; q++)
                    sum[q] = sum[q] + __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, t[q][j >> 2])));
            } else {
#pragma unroll
                for (int q = 0; q < NQ; q++) sum[q] = sum[q] + lt[q * m16 + j * 16 + (int)c];
            }
        }
    }
}

// a row of at most MG * 16 bytes held as words (M <= 32 MG); EXACT: M is 32 MG - 1 or 32 MG (the fast form)
template <int LOOKUP, int MG, int NQ, bool EXACT, int NV>
__device__ __forceinline__ void pq4_sum_words(float (&sum)[NQ], const float (&t)[NQ][NV], const float *lt, int M, const uint32_t (&c)[MG * 4])
{
#pragma unroll
    for (int wi = 0; wi < MG * 4; wi++) pq4_add_word<LOOKUP, NQ, NV>(sum, t, lt, M * 16, c[wi], wi, M, EXACT ? 32 * MG - 1 : 0);
}

// the row's P bytes at rowp, one at a time, as words; a lane that is not `active` reads nothing
template <int MG> __device__ __forceinline__ void pq4_load_row_bytes(uint32_t (&c)[MG * 4], const uint8_t *rowp, int P, bool active)
{
#pragma unroll
    for (int wi = 0; wi < MG * 4; wi++) c[wi] = 0u;
    if (active) {
#pragma unroll
        for (int b = 0; b < MG * 16; b++)
            if (b < P) c[b >> 2] |= (uint32_t)rowp[b] << (8 * (b & 3));
    }
}

// any M, tables in LDS: the row in pieces of 16 bytes straight from memory (VEC: P % 16 == 0 and 16-byte aligned rows)
template <int NQ, bool VEC>
__device__ __forceinline__ void pq4_sum_chunks(float (&sum)[NQ], const float *lt, int M, int P, const uint8_t *rowp, bool active)
{
    const float none[NQ][1] = {};
    for (int ch = 0; ch * 16 < P; ch++) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (active) {
            if (VEC) {
                const uint4 v = *reinterpret_cast<const uint4 *>(rowp + ch * 16);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
#pragma unroll
                for (int b = 0; b < 16; b++)
                    if (ch * 16 + b < P) w[b >> 2] |= (uint32_t)rowp[ch * 16 + b] << (8 * (b & 3));
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) pq4_add_word<PQ4_LDS, NQ, 1>(sum, none, lt, M * 16, w[i], ch * 4 + i, M, 0);
    }
}

// the queries' tables where the lookups find them: VGPR g of query q = tables[q][64 g + lane] (0 beyond M * 16), or LDS
template <int LOOKUP, int NQ, int NV>
__device__ __forceinline__ void pq4_load_tables(float (&t)[NQ][NV], float *lt, const float *tables, int m16, int tid, int nthreads)
{
    if constexpr (LOOKUP == PQ4_REG) {
        const int lane = tid & 63;
#pragma unroll
        for (int q = 0; q < NQ; q++)
#pragma unroll
            for (int g = 0; g < NV; g++) t[q][g] = g * 64 + lane < m16 ? tables[(int64_t)q * m16 + g * 64 + lane] : 0.f;
    } else {
#pragma unroll
        for (int q = 0; q < NQ; q++) t[q][0] = 0.f;
        for (int i = tid; i < NQ * m16; i += nthreads) lt[i] = tables[i];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The scan
// ---------------------------------------------------------------------------------------------------------------------------
struct Pq4Args {
    const float *tables; // [NQ][M * 16], queries slot .. slot + NQ - 1
    int M, P;
    const uint8_t *codes;
    int64_t row_begin, row_end;
    int slot;
    CandState cs;
    float *all_out; // indexed by absolute row - out_base (NQ == 1)
    int64_t out_base;
    int boot;
};

// MG > 0: M <= 32 MG, the row is held in MG * 4 registers (FAST: staged through LDS, P == 16 MG; else single bytes).
// MG == 0: any M, tables in LDS, the row in pieces from memory (FAST: 16-byte loads).
template <int LOOKUP, int MG, int NQ, bool FAST>
__global__ __launch_bounds__(PQ4_THREADS) void pq4_scan_kernel(Pq4Args a)
{
    static_assert(MG > 0 || LOOKUP == PQ4_LDS, "the register lookup needs the row's length at compile time");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NV = (LOOKUP == PQ4_REG) ? MG * 8 : 1;
    constexpr int PB = MG * 16; // FAST && MG > 0: bytes a row
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.M, P = a.P;
    float t[NQ][NV];
    float *lt = reinterpret_cast<float *>(smem);
    pq4_load_tables<LOOKUP, NQ, NV>(t, lt, a.tables, M * 16, tid, PQ4_THREADS);

    uint64_t tau[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) tau[q] = (a.all_out || a.boot) ? 0ull : a.cs.tau[a.slot + q];

    const int64_t nrows = a.row_end - a.row_begin;
    const int64_t ntiles = (nrows + 63) / 64;
    const int64_t tstride = (int64_t)gridDim.x * PQ4_WAVES;
    int64_t tile = (int64_t)blockIdx.x * PQ4_WAVES + wave;

    // the wave's staging slot (fast form): MG KiB behind the LDS tables
    const uint32_t stage_off = (LOOKUP == PQ4_LDS ? (uint32_t)(NQ * M * 64) : 0u) + (uint32_t)wave * (uint32_t)(PB * 64);
    const unsigned char *stage = smem + stage_off;
    const uint32_t stage_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem + stage_off;
    const unsigned char *last16 = a.codes + a.row_end * (int64_t)P - 16;
    // request i of a run: lane L brings bytes [1024 i + 16 L, + 16) of the run to the same place of the slot.  A run that ends
    // beyond the rows re-reads the last 16 bytes instead (rows past the end are dropped).  The grouped helpers move the source
    // by 1 KiB per request themselves: the sources are handed over pre-compensated.
    auto issue = [&](int64_t tl) {
        const unsigned char *src[MG > 0 ? MG : 1];
#pragma unroll
        for (int i = 0; i < MG; i++) {
            const unsigned char *p = a.codes + (a.row_begin + tl * 64) * (int64_t)P + i * 1024 + lane * 16;
            src[i] = p > last16 ? last16 : p;
        }
        if constexpr (MG == 1) {
            lds_dma16_noclobber<true>(src[0], stage_lds);
        } else if constexpr (MG == 2) {
            lds_dma16x2(src[0], src[1] - 1024, stage_lds);
        } else if constexpr (MG == 3) {
            lds_dma16x2(src[0], src[1] - 1024, stage_lds);
            lds_dma16_noclobber<true>(src[2], stage_lds + 2048u);
        } else if constexpr (MG == 4) {
            lds_dma16x4<true>(src[0], src[1] - 1024, src[2] - 2048, src[3] - 3072, stage_lds);
        }
        asm volatile("" ::: "memory");
    };

    if constexpr (FAST && MG > 0) {
        if (tile < ntiles) issue(tile);
    }
    for (; tile < ntiles; tile += tstride) {
        const int64_t row = a.row_begin + tile * 64 + lane;
        const bool active = row < a.row_end;
        float sum[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) sum[q] = 0.f;
        if constexpr (MG > 0) {
            uint32_t c[MG * 4];
            if constexpr (FAST) {
                wait_vmcnt<0>();
#pragma unroll
                for (int i = 0; i < MG; i++) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(stage + lane * PB + i * 16);
                    c[4 * i] = v.x; c[4 * i + 1] = v.y; c[4 * i + 2] = v.z; c[4 * i + 3] = v.w;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the slot is read before it is refilled
                if (tile + tstride < ntiles) issue(tile + tstride);
            } else {
                pq4_load_row_bytes<MG>(c, a.codes + row * (int64_t)P, P, active);
            }
            pq4_sum_words<LOOKUP, MG, NQ, FAST, NV>(sum, t, lt, M, c);
        } else {
            pq4_sum_chunks<NQ, FAST>(sum, lt, M, P, a.codes + row * (int64_t)P, active);
        }
        if (active) {
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                const float dist = adc_distance(sum[q]);
                if (a.all_out) {
                    a.all_out[row - a.out_base] = dist;
                } else {
                    const uint64_t ent = pack_entry(dist, (uint32_t)row);
                    uint64_t *list = a.cs.lists + (size_t)(a.slot + q) * a.cs.cap;
                    if (a.boot) {
                        list[row - a.row_begin] = ent;
                    } else if (ent < tau[q]) {
                        const uint32_t pos = atomicAdd(&a.cs.cnt[a.slot + q], 1u);
                        if (pos < a.cs.cap) list[pos] = ent;
                    }
                }
            }
        }
    }
}

template <int LOOKUP, int MG, int NQ, bool FAST> static void pq4_launch(const Pq4Args &a, hipStream_t s)
{
    const size_t shmem = (LOOKUP == PQ4_LDS ? (size_t)NQ * a.M * 64 : 0) + (FAST && MG > 0 ? (size_t)PQ4_WAVES * MG * 1024 : 0);
    if (shmem > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(pq4_scan_kernel<LOOKUP, MG, NQ, FAST>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    const int64_t ntiles = (a.row_end - a.row_begin + 63) / 64;
    int64_t blocks = (ntiles + PQ4_WAVES - 1) / PQ4_WAVES;
    if (blocks > PQ4_MAX_BLOCKS) blocks = PQ4_MAX_BLOCKS;
    hipLaunchKernelGGL((pq4_scan_kernel<LOOKUP, MG, NQ, FAST>), dim3((unsigned)blocks), dim3(PQ4_THREADS), shmem, s, a);
}

template <int LOOKUP, int MG, bool FAST> static void pq4_launch_g(const Pq4Args &a, int g, hipStream_t s)
{
    if (g == 1) return pq4_launch<LOOKUP, MG, 1, FAST>(a, s);
    if (g == 2) return pq4_launch<LOOKUP, MG, 2, FAST>(a, s);
    if constexpr (LOOKUP == PQ4_REG && MG <= 3) {
        if (g == 4) return pq4_launch<LOOKUP, MG, 4, FAST>(a, s);
    }
    throw std::logic_error("pq4 queries per pass"); // (never: pq4.hip groups by pq4_max_queries_per_pass)
}

template <int LOOKUP, bool FAST> static void pq4_launch_mg(const Pq4Args &a, int g, hipStream_t s)
{
    switch ((a.M + 31) / 32) {
    case 1: return pq4_launch_g<LOOKUP, 1, FAST>(a, g, s);
    case 2: return pq4_launch_g<LOOKUP, 2, FAST>(a, g, s);
    case 3: return pq4_launch_g<LOOKUP, 3, FAST>(a, g, s);
    default: return pq4_launch_g<LOOKUP, 4, FAST>(a, g, s);
    }
}

void launch_pq4_scan(const float *tables, int M, const uint8_t *codes, int64_t row_begin, int64_t row_end, int slot, int g, CandState cs,
                     bool boot, float *all_out, int64_t out_base, bool lds_lookup, hipStream_t s)
{
    if (row_end <= row_begin) return;
    Pq4Args a;
    a.tables = tables; a.M = M; a.P = pq4_row_bytes(M); a.codes = codes; a.row_begin = row_begin; a.row_end = row_end;
    a.slot = slot; a.cs = cs; a.all_out = all_out; a.out_base = out_base; a.boot = boot ? 1 : 0;
    const bool fast = a.P % 16 == 0 && (reinterpret_cast<uintptr_t>(codes) & 15) == 0;
    if (M > PQ4_REG_MAX_M) {
        if (fast) pq4_launch_g<PQ4_LDS, 0, true>(a, g, s);
        else pq4_launch_g<PQ4_LDS, 0, false>(a, g, s);
    } else if (!lds_lookup) {
        if (fast) pq4_launch_mg<PQ4_REG, true>(a, g, s);
        else pq4_launch_mg<PQ4_REG, false>(a, g, s);
    } else {
        if (fast) pq4_launch_mg<PQ4_LDS, true>(a, g, s);
        else pq4_launch_g<PQ4_LDS, 0, false>(a, g, s);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Exact entries of `count` evenly spaced rows of [0, n) (the sampled admission threshold): one lane per sampled row, its bytes
// one at a time, scored through the scan's own row sums.  The loop is uniform over a wave (ds_bpermute: every lane stays on).
// ---------------------------------------------------------------------------------------------------------------------------
template <int LOOKUP, int MG>
__global__ __launch_bounds__(PQ4_THREADS) void pq4_sample_kernel(const float *table, int M, int P, const uint8_t *codes, int64_t n,
                                                                 uint32_t count, uint64_t *out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NV = (LOOKUP == PQ4_REG) ? MG * 8 : 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane(tid & ~63);
    float t[1][NV];
    float *lt = reinterpret_cast<float *>(smem);
    pq4_load_tables<LOOKUP, 1, NV>(t, lt, table, M * 16, tid, PQ4_THREADS);
    for (uint32_t i0 = blockIdx.x * PQ4_THREADS + wbase; i0 < count; i0 += gridDim.x * PQ4_THREADS) {
        const uint32_t i = i0 + lane;
        const bool active = i < count;
        const int64_t row = active ? (int64_t)(((uint64_t)i * (uint64_t)n) / count) : 0; // i, n < 2^32
        float sum[1] = {0.f};
        if constexpr (MG > 0) {
            uint32_t c[MG * 4];
            pq4_load_row_bytes<MG>(c, codes + row * (int64_t)P, P, active);
            pq4_sum_words<LOOKUP, MG, 1, false, NV>(sum, t, lt, M, c);
        } else {
            pq4_sum_chunks<1, false>(sum, lt, M, P, codes + row * (int64_t)P, active);
        }
        if (active) out[i] = pack_entry(adc_distance(sum[0]), (uint32_t)row);
    }
}

void launch_pq4_sample(const float *table, int M, const uint8_t *codes, int64_t n, uint32_t count, uint64_t *out, bool lds_lookup,
                       hipStream_t s)
{
    if (count == 0) return;
    const int P = pq4_row_bytes(M);
    uint32_t blocks = (count + PQ4_THREADS - 1) / PQ4_THREADS;
    if (blocks > PQ4_MAX_BLOCKS) blocks = PQ4_MAX_BLOCKS;
    const dim3 grid(blocks), block(PQ4_THREADS);
    if (lds_lookup || M > PQ4_REG_MAX_M) {
        const size_t shmem = (size_t)M * 64;
        if (shmem > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(pq4_sample_kernel<PQ4_LDS, 0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)shmem);
        hipLaunchKernelGGL((pq4_sample_kernel<PQ4_LDS, 0>), grid, block, shmem, s, table, M, P, codes, n, count, out);
        return;
    }
    switch ((M + 31) / 32) {
    case 1: hipLaunchKernelGGL((pq4_sample_kernel<PQ4_REG, 1>), grid, block, 0, s, table, M, P, codes, n, count, out); break;
    case 2: hipLaunchKernelGGL((pq4_sample_kernel<PQ4_REG, 2>), grid, block, 0, s, table, M, P, codes, n, count, out); break;
    case 3: hipLaunchKernelGGL((pq4_sample_kernel<PQ4_REG, 3>), grid, block, 0, s, table, M, P, codes, n, count, out); break;
    default: hipLaunchKernelGGL((pq4_sample_kernel<PQ4_REG, 4>), grid, block, 0, s, table, M, P, codes, n, count, out); break;
    }
}

} // namespace lb
