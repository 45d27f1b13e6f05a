// kernels_sq8.hip -- scalar-quantised uint8 codes (store.SQ8Encoder, internal/store/scalar_quantization.go): per-dimension
// bounds, encode / decode, the integer distance S = sum (a_i - b_i)^2 (simd.EuclideanSQ8Generic, internal/simd/sq8.go:45-66)
// and the exact k-NN over it.
//
// Rows lie at a stride of dims rounded up to 16 bytes, pad bytes zero on both sides of every sum, so every dims takes the
// same kernels.  The distance pass: a tile is 256 rows, one lane owns a row.  A chunk is 4 pieces of 16 bytes of each of the
// tile's rows, fetched coalesced (consecutive lanes read consecutive pieces of the row-major codes) into an LDS tile whose row
// stride is 5 pieces: odd in 16-byte slots, so the 16 lanes that one ds_read_b128 cycle serves (distinct modulo 16) fall on 16
// distinct slots.  The QT queries' bytes lie in LDS and are read wave-uniform (broadcast).  x.q comes from v_dot4_u32_u8 and
// S = |x|^2 + |q|^2 - 2 x.q in integers: at most 65025 * 8192 < 2^30, nothing wraps.  Under a row list (a filtered search's
// ascending uint32 list of visible rows) position i of a tile is row list[pos0 + i]: the tile's 256 ids are staged into LDS first,
// one coalesced read of the list, and the pieces and the norm are gathered at them; S is then indexed by position.
//
// A search writes S once, as int32 [nq][n], and selects on that array by counting (lb_countsel.h states the method): a row is
// up to 8 KiB of codes and 4 bytes of S.  The histogram is a radix one: three (hist, digit) rounds over the digits of S (bits
// 31..21, 20..10, 9..0), each over the rows whose higher digits equal the ones found so far; after the third t is the k-th
// smallest S.  The count and emit kernels here read S; the scan and the finish are kernels_countsel.hip's.
#include "lb_countsel.h"
#include "lb_exact.h"

#include <cfloat>
#include <climits>
#include <type_traits>

namespace lb {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int SQ8_ROWS = COUNTSEL_ROWS;
constexpr int SQ8_CH = 4;                    // 16-byte pieces of a row per chunk
constexpr int SQ8_LD = SQ8_CH + 1;           // LDS row stride in pieces
constexpr size_t SQ8_LDS_BUDGET = 64 * 1024; // dynamic LDS a launch may ask for without opting in to more

// ---- bounds -----------------------------------------------------------------------------------------------------------
// TrainSQ8Encoder (scalar_quantization.go:99-118): min and max start at row 0 and later rows replace them through v < min /
// v > max only, so a NaN in a later row is ignored and a NaN in row 0 stays.  Lanes own dimensions, workgroup (x, y) owns
// rows [y * per, (y + 1) * per): its partial starts at +inf / -inf, which no comparison ever prefers to a bound.
__global__ __launch_bounds__(256) void sq8_bounds_seed_kernel(const float *X, int dims, float *state)
{
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d < dims) {
        state[d] = X[d];
        state[dims + d] = X[d];
    }
}

__global__ __launch_bounds__(256) void sq8_bounds_part_kernel(const float *X, int64_t n, int dims, int64_t per, float *part)
{
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= dims) return;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < n ? r0 + per : n;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    for (int64_t r = r0; r < r1; r++) {
        const float v = X[r * dims + d];
        if (v < mn) mn = v;
        if (v > mx) mx = v;
    }
    part[((int64_t)blockIdx.y * 2) * dims + d] = mn;
    part[((int64_t)blockIdx.y * 2 + 1) * dims + d] = mx;
}

// the partials into the state, in the order of their rows
__global__ __launch_bounds__(256) void sq8_bounds_fold_kernel(const float *part, int parts, int dims, float *state)
{
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= dims) return;
    float mn = state[d], mx = state[dims + d];
    for (int p = 0; p < parts; p++) {
        const float a = part[((int64_t)p * 2) * dims + d], b = part[((int64_t)p * 2 + 1) * dims + d];
        if (a < mn) mn = a;
        if (b > mx) mx = b;
    }
    state[d] = mn;
    state[dims + d] = mx;
}

// ---- codec ------------------------------------------------------------------------------------------------------------
// EncodeInto (scalar_quantization.go:155-170).  The clamp is the reference's two comparisons, so a NaN passes both; the
// product is a subtraction and a multiplication, each rounded once.  uint8(product) is Go's conversion as amd64 performs it
// (truncate to int32, keep the low byte; a NaN or a product beyond int32 converts to 0x80000000, whose low byte is 0).
__device__ __forceinline__ uint32_t sq8_code(float v, float mn, float mx, float scale)
{
#pragma clang fp contract(off)
    if (v < mn) v = mn;
    else if (v > mx) v = mx;
    const float d = v - mn;
    const float p = d * scale;
    if (!(p >= -2147483648.0f && p < 2147483648.0f)) return 0u;
    return (uint32_t)(int32_t)p & 255u;
}

// one lane per four codes of the strided output: one 4-byte store
__global__ __launch_bounds__(256) void sq8_encode_kernel(const float *X, int64_t n, int dims, int stride, const float *mn, const float *mx,
                                                         const float *scale, uint32_t *codes)
{
    const int sw = stride >> 2;
    const int64_t total = n * sw;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / sw;
        const int i0 = (int)(e - r * sw) * 4;
        uint32_t w = 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = i0 + b;
            if (i < dims) w |= sq8_code(X[r * dims + i], mn[i], mx[i], scale[i]) << (8 * b);
        }
        codes[e] = w;
    }
}

// DecodeInto (scalar_quantization.go:180-184): min + float32(q) * invScale, the product rounded before the sum
__device__ __forceinline__ float sq8_value(uint32_t q, float mn, float inv)
{
#pragma clang fp contract(off)
    const float p = (float)q * inv;
    return mn + p;
}

__global__ __launch_bounds__(256) void sq8_decode_kernel(const uint8_t *codes, int64_t n, int dims, int cstride, const float *mn,
                                                         const float *inv, float *out)
{
    const int64_t total = n * dims;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / dims;
        const int i = (int)(e - r * dims);
        out[e] = sq8_value(codes[r * cstride + i], mn[i], inv[i]);
    }
}

__global__ __launch_bounds__(256) void sq8_restride_kernel(const uint8_t *src, int sstride, uint8_t *dst, int dstride, int width, int64_t n)
{
    const int64_t total = n * dstride;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / dstride;
        const int c = (int)(e - r * dstride);
        dst[e] = c < width ? src[r * sstride + c] : (uint8_t)0;
    }
}

__device__ __forceinline__ uint32_t sq8_dot16(const u32x4 a, const u32x4 b, uint32_t acc)
{
    acc = __builtin_amdgcn_udot4(a.x, b.x, acc, false);
    acc = __builtin_amdgcn_udot4(a.y, b.y, acc, false);
    acc = __builtin_amdgcn_udot4(a.z, b.z, acc, false);
    acc = __builtin_amdgcn_udot4(a.w, b.w, acc, false);
    return acc;
}

// one wave per row: norms[r] = sum of the squares of its bytes
__global__ __launch_bounds__(256) void sq8_norms_kernel(const u32x4 *codes, int64_t n, int P, int32_t *norms)
{
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
        uint32_t s = 0u;
        for (int p = lane; p < P; p += 64) {
            const u32x4 v = codes[r * P + p];
            s = sq8_dot16(v, v, s);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) norms[r] = (int32_t)s;
    }
}

// ---- the distance pass ------------------------------------------------------------------------------------------------
constexpr size_t sq8_ids_lds(bool mapped) { return mapped ? (size_t)SQ8_ROWS * 4 : 0; } // the staged ids, in front of the tile

// workgroup (x, y): tiles [x * tpb, (x + 1) * tpb) of the rows [row0, row0 + n), queries [y * QT, (y + 1) * QT); MAPPED: of the
// n positions of rowmap (row0 = 0).  The list is the last kernel argument, behind the parent's: the unmapped form never loads it
// and its argument block, and with it its scalar register allocation, is what it was.
template <int QT, bool MAPPED>
__global__ __launch_bounds__(SQ8_ROWS) void sq8_dist_kernel(Sq8Dist a, int tpb, const uint32_t *rowmap)
{
    extern __shared__ __attribute__((aligned(16))) u32x4 sq8_smem[];
    u32x4 *lrow = sq8_smem;                 // [SQ8_ROWS][SQ8_LD]
    if constexpr (MAPPED) lrow += sq8_ids_lds(true) / 16; // the tile's row ids u32[SQ8_ROWS] lie in front of it
    u32x4 *lq = lrow + SQ8_ROWS * SQ8_LD;   // [QT][Pq], zero past P; a slot past nq repeats the last query
    const int tid = threadIdx.x;
    const int P = a.stride >> 4, nchunks = (P + SQ8_CH - 1) / SQ8_CH, Pq = nchunks * SQ8_CH;
    const int q0 = blockIdx.y * QT;
    const u32x4 *codes = reinterpret_cast<const u32x4 *>(a.codes);
    const u32x4 *Q = reinterpret_cast<const u32x4 *>(a.Q);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int idx = tid; idx < QT * Pq; idx += SQ8_ROWS) {
        const int j = idx / Pq, p = idx - j * Pq;
        const int q = q0 + j < a.nq ? q0 + j : a.nq - 1;
        lq[idx] = p < P ? Q[(int64_t)q * P + p] : zero;
    }
    int32_t qn[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) qn[j] = a.qn[q0 + j < a.nq ? q0 + j : a.nq - 1];
    __syncthreads();
    const int64_t ntiles = (a.n + SQ8_ROWS - 1) / SQ8_ROWS;
    const int64_t t0 = (int64_t)blockIdx.x * tpb, t1 = t0 + tpb < ntiles ? t0 + tpb : ntiles;
    for (int64_t tile = t0; tile < t1; tile++) {
        const int64_t pos0 = tile * SQ8_ROWS;
        uint32_t acc[QT];
#pragma unroll
        for (int j = 0; j < QT; j++) acc[j] = 0u;
        if constexpr (MAPPED) { // (the chunk loop's barriers order the reads of the ids before the next tile's writes)
            reinterpret_cast<uint32_t *>(sq8_smem)[tid] = pos0 + tid < a.n ? rowmap[pos0 + tid] : 0u;
            __syncthreads();
        }
        for (int c = 0; c < nchunks; c++) {
#pragma unroll
            for (int i = 0; i < SQ8_CH; i++) {
                const int ch = tid + SQ8_ROWS * i;
                const int r = ch / SQ8_CH, pv = ch - r * SQ8_CH;
                const int p = c * SQ8_CH + pv;
                u32x4 v = zero;
                // a plain load: the other query tiles find the row in L2 / MALL
                if (pos0 + r < a.n && p < P) v = codes[(MAPPED ? (int64_t)reinterpret_cast<const uint32_t *>(sq8_smem)[r] : a.row0 + pos0 + r) * P + p];
                lrow[r * SQ8_LD + pv] = v;
            }
            __syncthreads();
            u32x4 x[SQ8_CH];
#pragma unroll
            for (int w = 0; w < SQ8_CH; w++) x[w] = lrow[tid * SQ8_LD + w];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < QT; j++) {
                const u32x4 *q = lq + j * Pq + c * SQ8_CH;
#pragma unroll
                for (int w = 0; w < SQ8_CH; w++) acc[j] = sq8_dot16(x[w], q[w], acc[j]);
            }
        }
        if (pos0 + tid < a.n) {
            const int32_t xn = a.norms[MAPPED ? (int64_t)reinterpret_cast<const uint32_t *>(sq8_smem)[tid] : a.row0 + pos0 + tid];
#pragma unroll
            for (int j = 0; j < QT; j++)
                if (q0 + j < a.nq) a.out[(int64_t)(q0 + j) * a.n + pos0 + tid] = xn + qn[j] - 2 * (int32_t)acc[j];
        }
    }
}

// gathered rows, one lane per pair, sequential in i: S (SQ8DistanceFast, scalar_quantization.go:208-216) and, where asked,
// SQ8EuclideanDistance (:192-203): an f32 sum of diff * diff over the decoded values, then float32(sqrt(float64(sum)))
__global__ __launch_bounds__(256) void sq8_rerank_kernel(const uint8_t *codes, int stride, int dims, int64_t ntotal, const uint8_t *qcode,
                                                         const int64_t *rows, int64_t n, const float *mn, const float *inv, int32_t *out_s,
                                                         float *out_e)
{
#pragma clang fp contract(off)
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t row = rows[e];
        if (row < 0 || row >= ntotal) {
            out_s[e] = INT_MAX;
            if (out_e) out_e[e] = FLT_MAX;
            continue;
        }
        const uint8_t *x = codes + row * stride;
        int32_t s = 0;
        for (int i = 0; i < dims; i++) {
            const int32_t d = (int32_t)qcode[i] - (int32_t)x[i];
            s += d * d;
        }
        out_s[e] = s;
        if (out_e) {
            Acc<ORDER_SEQ> sum;
            sum.zero();
            for (int i = 0; i < dims; i++) {
                const float v1 = sq8_value(qcode[i], mn[i], inv[i]), v2 = sq8_value(x[i], mn[i], inv[i]);
                const float diff = v1 - v2;
                sum.add_tail(diff * diff);
            }
            out_e[e] = (float)sqrt((double)sum.total());
        }
    }
}

// ---- top-k by counting ------------------------------------------------------------------------------------------------
// the digit of pass 0, 1, 2 and the digits above it
__device__ __forceinline__ uint32_t sq8_digit(uint32_t s, int pass) { return pass == 0 ? s >> 21 : pass == 1 ? (s >> 10) & 2047u : s & 1023u; }
__device__ __forceinline__ uint32_t sq8_above(uint32_t s, int pass) { return pass == 0 ? 0u : pass == 1 ? s >> 21 : s >> 10; }

// workgroup (x, y) owns rows [x * tpb * 256, (x + 1) * tpb * 256) of query y
__device__ __forceinline__ void sq8_range(const Sq8Select &a, int64_t &r0, int64_t &r1)
{
    r0 = (int64_t)blockIdx.x * a.tpb * SQ8_ROWS;
    r1 = r0 + (int64_t)a.tpb * SQ8_ROWS;
    if (r1 > a.n) r1 = a.n;
}

__global__ __launch_bounds__(SQ8_ROWS) void sq8_hist_kernel(Sq8Select a, int pass)
{
    __shared__ uint32_t lh[SQ8_RADIX_BINS];
    const int tid = threadIdx.x, q = blockIdx.y;
    const uint32_t prefix = pass ? a.thr[2 * q] : 0u;
    if (prefix == 0x7fffffffu) return; // fewer than k rows: nothing to find (wave-uniform)
    for (int i = tid; i < SQ8_RADIX_BINS; i += SQ8_ROWS) lh[i] = 0u;
    __syncthreads();
    const int32_t *S = a.S + (int64_t)q * a.n;
    int64_t r0, r1;
    sq8_range(a, r0, r1);
    for (int64_t pos = r0 + tid; pos < r1; pos += SQ8_ROWS) {
        const uint32_t s = (uint32_t)S[pos];
        if (sq8_above(s, pass) == prefix) atomicAdd(&lh[sq8_digit(s, pass)], 1u);
    }
    __syncthreads();
    for (int i = tid; i < SQ8_RADIX_BINS; i += SQ8_ROWS) {
        const uint32_t v = lh[i];
        if (v) atomicAdd(&a.hist[(int64_t)q * SQ8_RADIX_BINS + i], v);
    }
}

// thr[q] = {digits so far, rank wanted among the rows that share them}; leaves the histogram zero for the next pass
__global__ __launch_bounds__(256) void sq8_digit_kernel(Sq8Select a, int pass)
{
    __shared__ uint32_t part[256];
    const int tid = threadIdx.x, q = blockIdx.x;
    constexpr int per = SQ8_RADIX_BINS / 256;
    uint32_t *h = a.hist + (int64_t)q * SQ8_RADIX_BINS;
    const uint32_t prefix = pass ? a.thr[2 * q] : 0u, want = pass ? a.thr[2 * q + 1] : (uint32_t)a.k;
    if (prefix == 0x7fffffffu) return; // (wave-uniform; the histogram was left zero)
    uint32_t s = 0;
    for (int b = tid * per; b < (tid + 1) * per; b++) s += h[b];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint32_t bin = 0, need = 0;
        const bool found = countsel_find(h, part, per, want, bin, need);
        a.thr[2 * q] = found ? (prefix << (pass == 2 ? 10 : 11)) | bin : 0x7fffffffu;
        a.thr[2 * q + 1] = need;
    }
    __syncthreads();
    for (int b = tid * per; b < (tid + 1) * per; b++) h[b] = 0u;
}

__global__ __launch_bounds__(SQ8_ROWS) void sq8_count_kernel(Sq8Select a)
{
    __shared__ uint32_t lc[2];
    const int tid = threadIdx.x, q = blockIdx.y;
    if (tid < 2) lc[tid] = 0u;
    __syncthreads();
    const uint32_t t = a.thr[2 * q];
    const int32_t *S = a.S + (int64_t)q * a.n;
    int64_t r0, r1;
    sq8_range(a, r0, r1);
    uint32_t clt = 0, ceq = 0;
    for (int64_t pos = r0 + tid; pos < r1; pos += SQ8_ROWS) {
        const uint32_t s = (uint32_t)S[pos];
        clt += s < t;
        ceq += s == t;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        clt += __shfl_xor(clt, off);
        ceq += __shfl_xor(ceq, off);
    }
    if ((tid & 63) == 0) {
        atomicAdd(&lc[0], clt);
        atomicAdd(&lc[1], ceq);
    }
    __syncthreads();
    if (tid < 2) a.cnt[((int64_t)q * a.nblk + blockIdx.x) * 2 + tid] = lc[tid];
}

__global__ __launch_bounds__(SQ8_ROWS) void sq8_emit_kernel(Sq8Select a)
{
    __shared__ uint32_t run[2];     // slots used so far: below t, at t
    __shared__ uint32_t wcnt[4][2]; // per wave of the tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.y;
    if (tid < 2) run[tid] = a.cnt[((int64_t)q * a.nblk + blockIdx.x) * 2 + tid];
    const uint32_t t = a.thr[2 * q], need = a.thr[2 * q + 1], below = a.tot[q];
    const int32_t *S = a.S + (int64_t)q * a.n;
    int64_t r0, r1;
    sq8_range(a, r0, r1);
    const unsigned long long lower = (1ull << lane) - 1ull;
    __syncthreads();
    for (int64_t pos0 = r0; pos0 < r1; pos0 += SQ8_ROWS) {
        const int64_t pos = pos0 + tid;
        const bool mine = pos < r1;
        const uint32_t s = mine ? (uint32_t)S[pos] : 0u;
        const bool lt = mine && s < t, eq = mine && s == t;
        const unsigned long long blt = __ballot(lt), beq = __ballot(eq);
        if (lane == 0) {
            wcnt[wave][0] = (uint32_t)__popcll(blt);
            wcnt[wave][1] = (uint32_t)__popcll(beq);
        }
        __syncthreads();
        const uint32_t slot = countsel_slot(lt, eq, blt, beq, run, &wcnt[0][0], wave, lower, below, need, a.k);
        if (slot != COUNTSEL_NO_SLOT) a.keys[(int64_t)q * a.k + slot] = ((uint64_t)s << 32) | (uint64_t)pos;
        __syncthreads();
        if (tid < 2) run[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
        __syncthreads(); // the next tile rewrites wcnt
    }
}

// the staged ids (under a list), the tile and the queries
size_t sq8_dist_lds(int stride, int qt, bool mapped)
{
    const int P = stride >> 4, Pq = (P + SQ8_CH - 1) / SQ8_CH * SQ8_CH;
    return sq8_ids_lds(mapped) + ((size_t)SQ8_ROWS * SQ8_LD + (size_t)qt * Pq) * 16;
}

// the query tile of a launch (pick_qt) within the LDS budget
int sq8_qt(int nq, int stride, bool mapped)
{
    return pick_qt(nq, [&](int qt) { return sq8_dist_lds(stride, qt, mapped) <= SQ8_LDS_BUDGET; });
}

} // namespace

int sq8_bounds_parts(int64_t n) { return (int)grid_cap((n + 63) / 64, 256); }

void launch_sq8_bounds_seed(const float *X, int dims, float *state, hipStream_t s)
{
    sq8_bounds_seed_kernel<<<dim3((unsigned)((dims + 255) / 256)), dim3(256), 0, s>>>(X, dims, state);
}

void launch_sq8_bounds_fold(const float *X, int64_t n, int dims, float *part, float *state, hipStream_t s)
{
    if (n <= 0) return;
    const int parts = sq8_bounds_parts(n);
    const int64_t per = (n + parts - 1) / parts;
    const unsigned gx = (unsigned)((dims + 255) / 256);
    sq8_bounds_part_kernel<<<dim3(gx, (unsigned)parts), dim3(256), 0, s>>>(X, n, dims, per, part);
    sq8_bounds_fold_kernel<<<dim3(gx), dim3(256), 0, s>>>(part, parts, dims, state);
}

void launch_sq8_encode(const float *X, int64_t n, int dims, const float *mn, const float *mx, const float *scale, uint8_t *codes,
                       hipStream_t s)
{
    if (n <= 0) return;
    const int stride = sq8_stride(dims);
    sq8_encode_kernel<<<dim3((unsigned)grid_cap((n * (stride >> 2) + 255) / 256, 1 << 20)), dim3(256), 0, s>>>(
        X, n, dims, stride, mn, mx, scale, reinterpret_cast<uint32_t *>(codes));
}

void launch_sq8_decode(const uint8_t *codes, int64_t n, int dims, int cstride, const float *mn, const float *inv, float *out,
                       hipStream_t s)
{
    if (n <= 0) return;
    sq8_decode_kernel<<<dim3((unsigned)grid_cap((n * dims + 255) / 256, 1 << 20)), dim3(256), 0, s>>>(codes, n, dims, cstride, mn, inv, out);
}

void launch_sq8_restride(const uint8_t *src, int sstride, uint8_t *dst, int dstride, int width, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    sq8_restride_kernel<<<dim3((unsigned)grid_cap((n * dstride + 255) / 256, 1 << 20)), dim3(256), 0, s>>>(src, sstride, dst, dstride, width, n);
}

void launch_sq8_norms(const uint8_t *codes, int64_t n, int stride, int32_t *norms, hipStream_t s)
{
    if (n <= 0) return;
    sq8_norms_kernel<<<dim3((unsigned)grid_cap((n + 3) / 4, 1 << 16)), dim3(256), 0, s>>>(reinterpret_cast<const u32x4 *>(codes), n, stride >> 4,
                                                                                         norms);
}

void launch_sq8_dist(const Sq8Dist &a, hipStream_t s, const uint32_t *rowmap)
{
    if (a.n <= 0 || a.nq <= 0) return;
    int nblk, tpb;
    countsel_plan(a.n, SQ8_MAX_BLOCKS, &nblk, &tpb);
    const bool mapped = rowmap != nullptr;
    const int qt = sq8_qt(a.nq, a.stride, mapped);
    const size_t lds = sq8_dist_lds(a.stride, qt, mapped);
    const dim3 grid((unsigned)nblk, (unsigned)((a.nq + qt - 1) / qt));
    with_qt(qt, [&](auto q) {
        if (mapped) sq8_dist_kernel<decltype(q)::value, true><<<grid, dim3(SQ8_ROWS), lds, s>>>(a, tpb, rowmap);
        else sq8_dist_kernel<decltype(q)::value, false><<<grid, dim3(SQ8_ROWS), lds, s>>>(a, tpb, nullptr);
    });
}

void launch_sq8_rerank(const uint8_t *codes, int stride, int dims, int64_t ntotal, const uint8_t *qcode, const int64_t *rows, int64_t n,
                       const float *mn, const float *inv, int32_t *out_s, float *out_euclid, hipStream_t s)
{
    if (n <= 0) return;
    sq8_rerank_kernel<<<dim3((unsigned)grid_cap((n + 255) / 256, 1 << 16)), dim3(256), 0, s>>>(codes, stride, dims, ntotal, qcode, rows, n, mn,
                                                                                              inv, out_s, out_euclid);
}

void launch_sq8_hist(const Sq8Select &a, int pass, hipStream_t s)
{
    sq8_hist_kernel<<<dim3((unsigned)a.nblk, (unsigned)a.nq), dim3(SQ8_ROWS), 0, s>>>(a, pass);
}
void launch_sq8_digit(const Sq8Select &a, int pass, hipStream_t s) { sq8_digit_kernel<<<dim3((unsigned)a.nq), dim3(256), 0, s>>>(a, pass); }
void launch_sq8_count(const Sq8Select &a, hipStream_t s)
{
    sq8_count_kernel<<<dim3((unsigned)a.nblk, (unsigned)a.nq), dim3(SQ8_ROWS), 0, s>>>(a);
}
void launch_sq8_emit(const Sq8Select &a, hipStream_t s)
{
    sq8_emit_kernel<<<dim3((unsigned)a.nblk, (unsigned)a.nq), dim3(SQ8_ROWS), 0, s>>>(a);
}

} // namespace lb
