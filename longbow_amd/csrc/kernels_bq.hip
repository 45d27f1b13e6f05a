// kernels_bq.hip -- binary-quantised codes (store.BQEncoder, internal/store/binary_quantization.go): sign-bit encode / decode,
// Hamming distances (simd.HammingDistance, internal/simd/simd_bitops.go:40-55) and the exact k-NN by counting.
//
// The distance pass, shared by every kernel below: a tile is 256 rows, one lane owns a row.  A chunk is CW words of each of
// the tile's rows, fetched as coalesced 8-B words (consecutive lanes read consecutive words of the row-major codes) into an LDS
// tile with an odd row stride of CW + 1 words, from which each lane reads its own row's CW words into registers
// (conflict-free ds_read_b64).  The QT queries' words lie in LDS and are read wave-uniform (broadcast).  W <= 16 is one
// chunk (CW = 4, 8, 12 or 16: the words stay in registers for all QT queries); wider rows walk chunks of 8 words.  Words past
// W are zero on both sides.  Distances sum whole words, so pad bits a caller stored count (as in the reference).
//
// Under a row filter a search walks the ascending uint32 list of visible rows: local position i of a tile is row
// list[pos0 + i].  The tile's 256 row ids are staged into LDS first, one coalesced 1 KiB read of the list, and the chunk loop
// takes them from there.  The gathers are then runs of CW (at most W) consecutive words per row, 96 B at 768 bits: partial 128-B
// lines where the unmapped form reads whole ones.
//
// Top-k needs no candidate list: the distance takes at most 64*W + 1 <= 8193 values, so the search selects by counting
// (lb_countsel.h states the method: hist, thresh, count, scan, emit, finish).  The hist, count and emit kernels here recompute
// the distances tile by tile; the scan and the finish are kernels_countsel.hip's.
#include "lb_countsel.h"

#include <cfloat>
#include <type_traits>

namespace lb {

namespace {

constexpr int BQ_ROWS = COUNTSEL_ROWS;
constexpr size_t BQ_LDS_BUDGET = 64 * 1024; // dynamic LDS a launch may ask for without opting in to more

// ---- codec ------------------------------------------------------------------------------------------------------------
// One wave per word: 64 lanes compare 64 consecutive f32 of a row, the ballot is the word.  v > 0 as the reference compares
// it (binary_quantization.go:41), on the bit pattern so that no denormal mode can change it: 0x00000001..0x7f800000.
__global__ __launch_bounds__(256) void bq_encode_kernel(const uint32_t *X, int64_t n, int dims, int W, uint64_t *codes)
{
    const int lane = threadIdx.x & 63;
    const int64_t nwords = n * W;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < nwords; u += (int64_t)gridDim.x * 4) {
        const int64_t r = u / W;
        const int i = (int)(u - r * W) * 64 + lane;
        uint32_t bits = 0;
        if (i < dims) bits = X[r * dims + i];
        const unsigned long long word = __ballot(bits - 1u < 0x7f800000u);
        if (lane == 0) codes[u] = word;
    }
}

__global__ __launch_bounds__(256) void bq_decode_kernel(const uint64_t *codes, int64_t n, int dims, int W, float *out)
{
    const int64_t total = n * dims;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / dims;
        const int i = (int)(e - r * dims);
        out[e] = ((codes[r * W + (i >> 6)] >> (i & 63)) & 1ull) ? 1.0f : -1.0f;
    }
}

// ---- the distance pass ------------------------------------------------------------------------------------------------
struct BqRows {
    const uint64_t *codes;
    int W;
    int64_t ntotal;      // MAPPED: rows outside [0, ntotal) are invalid
    const int64_t *rows; // MAPPED: the gathered list; else local index i is row i
};

__device__ __forceinline__ int bq_nchunks(int W, int CW) { return (W + CW - 1) / CW; }

// the QT queries' words -> lq[QT][Wq] (Wq = nchunks*CW), zero past W; a slot past nq repeats the last query
template <int CW, int QT>
__device__ __forceinline__ void bq_load_queries(const uint64_t *Q, int W, int q0, int nq, uint64_t *lq, int tid)
{
    const int Wq = bq_nchunks(W, CW) * CW;
    for (int idx = tid; idx < QT * Wq; idx += BQ_ROWS) {
        const int j = idx / Wq, w = idx - j * Wq;
        const int q = q0 + j < nq ? q0 + j : nq - 1;
        lq[idx] = w < W ? Q[(int64_t)q * W + w] : 0ull;
    }
}

// acc[j] = Hamming distance of local row pos0 + tid to query slot j; rows at or past pos_end (and invalid gathered rows) read as
// zero words.  Ends with the LDS tile free again.  Returns whether this lane's row is a real one.
template <int CW, int QT, bool MAPPED>
__device__ __forceinline__ bool bq_tile(const BqRows &a, int64_t pos0, int64_t pos_end, uint64_t *lrow, const uint64_t *lq, int tid,
                                        int (&acc)[QT])
{
    constexpr int LD = CW + 1;
    const int W = a.W, nchunks = bq_nchunks(W, CW), Wq = nchunks * CW;
#pragma unroll
    for (int j = 0; j < QT; j++) acc[j] = 0;
    bool mine = pos0 + tid < pos_end;
    if (MAPPED && mine) {
        const int64_t row = a.rows[pos0 + tid];
        mine = row >= 0 && row < a.ntotal;
    }
    for (int c = 0; c < nchunks; c++) {
#pragma unroll
        for (int i = 0; i < CW; i++) {
            const int ch = tid + BQ_ROWS * i;
            const int r = ch / CW, wv = ch - r * CW;
            const int w = c * CW + wv;
            int64_t row = pos0 + r;
            bool ok = row < pos_end && w < W;
            if (MAPPED && ok) {
                row = a.rows[row];
                ok = row >= 0 && row < a.ntotal;
            }
            uint64_t v = 0ull;
            if (ok) v = a.codes[row * W + w]; // a plain load: the other query tiles and the next pass find the row in L2 / MALL
            lrow[r * LD + wv] = v;
        }
        __syncthreads();
        uint64_t x[CW];
#pragma unroll
        for (int w = 0; w < CW; w++) x[w] = lrow[tid * LD + w];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QT; j++) {
            const uint64_t *q = lq + j * Wq + c * CW;
            int s = 0;
#pragma unroll
            for (int w = 0; w < CW; w++) s += __popcll(x[w] ^ q[w]);
            acc[j] += s;
        }
    }
    return mine;
}

constexpr int BQ_IDS_WORDS = BQ_ROWS / 2; // u64 words of LDS the staged row ids of a tile take, in front of the tile

// bq_tile under a filtered search's list: local row pos0 + i is row list[pos0 + i], every entry a stored row.  The ids go to the
// BQ_IDS_WORDS in front of lrow first; the chunk loop's barriers order their reads before the next tile's writes.  (A function
// of its own, and bq_tile left as it is: the unmapped kernels then stay the code they were, instruction for instruction.  The
// list is a parameter and not a field of BqRows, which is a kernel argument of bq_batch_kernel and bq_rerank_kernel.)
template <int CW, int QT>
__device__ __forceinline__ bool bq_tile_list(const BqRows &a, const uint32_t *list, int64_t pos0, int64_t pos_end, uint64_t *lrow,
                                             const uint64_t *lq, int tid, int (&acc)[QT])
{
    constexpr int LD = CW + 1;
    constexpr uint32_t NO_ROW = ~0u; // (rows are below 2^31)
    uint32_t *lid = reinterpret_cast<uint32_t *>(lrow - BQ_IDS_WORDS);
    const int W = a.W, nchunks = bq_nchunks(W, CW), Wq = nchunks * CW;
#pragma unroll
    for (int j = 0; j < QT; j++) acc[j] = 0;
    const bool mine = pos0 + tid < pos_end;
    lid[tid] = mine ? list[pos0 + tid] : NO_ROW;
    __syncthreads();
    for (int c = 0; c < nchunks; c++) {
#pragma unroll
        for (int i = 0; i < CW; i++) {
            const int ch = tid + BQ_ROWS * i;
            const int r = ch / CW, wv = ch - r * CW;
            const int w = c * CW + wv;
            const uint32_t id = lid[r]; // consecutive lanes: one word or consecutive ones (broadcast, no bank conflict)
            uint64_t v = 0ull;
            if (id != NO_ROW && w < W) v = a.codes[(int64_t)id * W + w];
            lrow[r * LD + wv] = v;
        }
        __syncthreads();
        uint64_t x[CW];
#pragma unroll
        for (int w = 0; w < CW; w++) x[w] = lrow[tid * LD + w];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QT; j++) {
            const uint64_t *q = lq + j * Wq + c * CW;
            int s = 0;
#pragma unroll
            for (int w = 0; w < CW; w++) s += __popcll(x[w] ^ q[w]);
            acc[j] += s;
        }
    }
    return mine;
}

// HammingDistanceBatch over stored rows [row0, row0 + n) (binary_quantization.go:56-60)
template <int CW>
__global__ __launch_bounds__(BQ_ROWS) void bq_batch_kernel(BqRows a, const uint64_t *qcode, int64_t row0, int64_t n, int32_t *out)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t bq_smem[];
    uint64_t *lrow = bq_smem;
    uint64_t *lq = lrow + BQ_ROWS * (CW + 1);
    const int tid = threadIdx.x;
    bq_load_queries<CW, 1>(qcode, a.W, 0, 1, lq, tid);
    __syncthreads();
    const int64_t ntiles = (n + BQ_ROWS - 1) / BQ_ROWS;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int acc[1];
        const int64_t pos0 = row0 + tile * BQ_ROWS;
        if (bq_tile<CW, 1, false>(a, pos0, row0 + n, lrow, lq, tid, acc)) out[pos0 - row0 + tid] = acc[0];
    }
}

// gathered rows: float32(distance) and ScoreToFloat32 (binary_quantization.go:69-71); rows outside [0, ntotal): FLT_MAX / 0
template <int CW>
__global__ __launch_bounds__(BQ_ROWS) void bq_rerank_kernel(BqRows a, const uint64_t *qcode, int64_t n, int dims, float *dist, float *score)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t bq_smem[];
    uint64_t *lrow = bq_smem;
    uint64_t *lq = lrow + BQ_ROWS * (CW + 1);
    const int tid = threadIdx.x;
    bq_load_queries<CW, 1>(qcode, a.W, 0, 1, lq, tid);
    __syncthreads();
    const int64_t ntiles = (n + BQ_ROWS - 1) / BQ_ROWS;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int acc[1];
        const int64_t pos0 = tile * BQ_ROWS;
        const bool ok = bq_tile<CW, 1, true>(a, pos0, n, lrow, lq, tid, acc);
        if (pos0 + tid < n) {
            dist[pos0 + tid] = ok ? (float)acc[0] : FLT_MAX;
            if (score) score[pos0 + tid] = ok ? 1.0f - (float)acc[0] / (float)dims : 0.0f;
        }
    }
}

// ---- top-k by counting ------------------------------------------------------------------------------------------------
// workgroup b owns tiles [b*tpb, (b+1)*tpb): contiguous rows, so that positions order across workgroups.  MAPPED: the rows are
// the a.n positions of a.rowmap, and the keys carry positions (the finish maps them back)
template <int CW, int QT, bool MAPPED>
__global__ __launch_bounds__(BQ_ROWS) void bq_hist_kernel(BqSearch a)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t bq_smem[];
    uint64_t *lrow = bq_smem;
    if constexpr (MAPPED) lrow += BQ_IDS_WORDS;
    uint64_t *lq = lrow + BQ_ROWS * (CW + 1);
    const int nbins = 64 * a.W + 1;
    uint32_t *lh = reinterpret_cast<uint32_t *>(lq + QT * bq_nchunks(a.W, CW) * CW);
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * QT;
    bq_load_queries<CW, QT>(a.Q, a.W, q0, a.nq, lq, tid);
    for (int i = tid; i < QT * nbins; i += BQ_ROWS) lh[i] = 0u;
    __syncthreads();
    const BqRows rows{a.codes, a.W, a.n, nullptr};
    const int64_t ntiles = (a.n + BQ_ROWS - 1) / BQ_ROWS;
    const int64_t t0 = (int64_t)blockIdx.x * a.tpb, t1 = t0 + a.tpb < ntiles ? t0 + a.tpb : ntiles;
    for (int64_t tile = t0; tile < t1; tile++) {
        int acc[QT];
        if (MAPPED ? bq_tile_list<CW, QT>(rows, a.rowmap, tile * BQ_ROWS, a.n, lrow, lq, tid, acc)
                   : bq_tile<CW, QT, false>(rows, tile * BQ_ROWS, a.n, lrow, lq, tid, acc)) {
#pragma unroll
            for (int j = 0; j < QT; j++)
                if (q0 + j < a.nq) atomicAdd(&lh[j * nbins + acc[j]], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < QT * nbins; i += BQ_ROWS) {
        const int j = i / nbins;
        const uint32_t v = lh[i];
        if (v && q0 + j < a.nq) atomicAdd(&a.hist[(int64_t)(q0 + j) * nbins + (i - j * nbins)], v);
    }
}

// thr[q] = {t, need}; fewer than k rows in all: t = 0x7fffffff (every row is below it), need = 0
__global__ __launch_bounds__(256) void bq_thresh_kernel(BqSearch a)
{
    __shared__ uint32_t part[256];
    const int tid = threadIdx.x, q = blockIdx.x;
    const int nbins = 64 * a.W + 1, per = (nbins + 255) / 256;
    const uint32_t *h = a.hist + (int64_t)q * nbins;
    const int b0 = tid * per, b1 = b0 + per < nbins ? b0 + per : nbins;
    uint32_t s = 0;
    for (int b = b0; b < b1; b++) s += h[b];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0x7fffffffu, need = 0;
        countsel_find(h, part, per, (uint32_t)a.k, t, need);
        a.thr[2 * q] = t;
        a.thr[2 * q + 1] = need;
    }
}

template <int CW, int QT, bool MAPPED>
__global__ __launch_bounds__(BQ_ROWS) void bq_count_kernel(BqSearch a)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t bq_smem[];
    uint64_t *lrow = bq_smem;
    if constexpr (MAPPED) lrow += BQ_IDS_WORDS;
    uint64_t *lq = lrow + BQ_ROWS * (CW + 1);
    uint32_t *lc = reinterpret_cast<uint32_t *>(lq + QT * bq_nchunks(a.W, CW) * CW); // [QT][2]
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * QT;
    bq_load_queries<CW, QT>(a.Q, a.W, q0, a.nq, lq, tid);
    if (tid < QT * 2) lc[tid] = 0u;
    uint32_t t[QT], clt[QT], ceq[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) {
        t[j] = a.thr[2 * (q0 + j < a.nq ? q0 + j : a.nq - 1)];
        clt[j] = 0u;
        ceq[j] = 0u;
    }
    __syncthreads();
    const BqRows rows{a.codes, a.W, a.n, nullptr};
    const int64_t ntiles = (a.n + BQ_ROWS - 1) / BQ_ROWS;
    const int64_t t0 = (int64_t)blockIdx.x * a.tpb, t1 = t0 + a.tpb < ntiles ? t0 + a.tpb : ntiles;
    for (int64_t tile = t0; tile < t1; tile++) {
        int acc[QT];
        const bool mine = MAPPED ? bq_tile_list<CW, QT>(rows, a.rowmap, tile * BQ_ROWS, a.n, lrow, lq, tid, acc)
                                 : bq_tile<CW, QT, false>(rows, tile * BQ_ROWS, a.n, lrow, lq, tid, acc);
#pragma unroll
        for (int j = 0; j < QT; j++) { // wave-uniform counts
            clt[j] += (uint32_t)__popcll(__ballot(mine && (uint32_t)acc[j] < t[j]));
            ceq[j] += (uint32_t)__popcll(__ballot(mine && (uint32_t)acc[j] == t[j]));
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int j = 0; j < QT; j++) {
            atomicAdd(&lc[2 * j], clt[j]);
            atomicAdd(&lc[2 * j + 1], ceq[j]);
        }
    }
    __syncthreads();
    if (tid < QT * 2 && q0 + (tid >> 1) < a.nq) a.cnt[((int64_t)(q0 + (tid >> 1)) * a.nblk + blockIdx.x) * 2 + (tid & 1)] = lc[tid];
}

template <int CW, int QT, bool MAPPED>
__global__ __launch_bounds__(BQ_ROWS) void bq_emit_kernel(BqSearch a)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t bq_smem[];
    uint64_t *lrow = bq_smem;
    if constexpr (MAPPED) lrow += BQ_IDS_WORDS;
    uint64_t *lq = lrow + BQ_ROWS * (CW + 1);
    uint32_t *run = reinterpret_cast<uint32_t *>(lq + QT * bq_nchunks(a.W, CW) * CW); // [QT][2] slots used so far: below t, at t
    uint32_t *wcnt = run + QT * 2;                                                     // [QT][4 waves][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.y * QT;
    bq_load_queries<CW, QT>(a.Q, a.W, q0, a.nq, lq, tid);
    if (tid < QT * 2) {
        const int q = q0 + (tid >> 1);
        run[tid] = q < a.nq ? a.cnt[((int64_t)q * a.nblk + blockIdx.x) * 2 + (tid & 1)] : 0u;
    }
    uint32_t t[QT], need[QT], below[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) {
        const int q = q0 + j < a.nq ? q0 + j : a.nq - 1;
        t[j] = a.thr[2 * q];
        need[j] = q0 + j < a.nq ? a.thr[2 * q + 1] : 0u;
        below[j] = a.tot[q];
    }
    __syncthreads();
    const BqRows rows{a.codes, a.W, a.n, nullptr};
    const int64_t ntiles = (a.n + BQ_ROWS - 1) / BQ_ROWS;
    const int64_t t0 = (int64_t)blockIdx.x * a.tpb, t1 = t0 + a.tpb < ntiles ? t0 + a.tpb : ntiles;
    const unsigned long long lower = (1ull << lane) - 1ull;
    for (int64_t tile = t0; tile < t1; tile++) {
        int acc[QT];
        const bool mine = MAPPED ? bq_tile_list<CW, QT>(rows, a.rowmap, tile * BQ_ROWS, a.n, lrow, lq, tid, acc)
                                 : bq_tile<CW, QT, false>(rows, tile * BQ_ROWS, a.n, lrow, lq, tid, acc);
#pragma unroll
        for (int j = 0; j < QT; j++) {
            const bool on = mine && q0 + j < a.nq;
            const unsigned long long blt = __ballot(on && (uint32_t)acc[j] < t[j]), beq = __ballot(on && (uint32_t)acc[j] == t[j]);
            if (lane == 0) {
                wcnt[(j * 4 + wave) * 2] = (uint32_t)__popcll(blt);
                wcnt[(j * 4 + wave) * 2 + 1] = (uint32_t)__popcll(beq);
            }
        }
        __syncthreads();
        const uint64_t pos = (uint64_t)(tile * BQ_ROWS + tid);
#pragma unroll
        for (int j = 0; j < QT; j++) {
            const bool on = mine && q0 + j < a.nq;
            const bool lt = on && (uint32_t)acc[j] < t[j], eq = on && (uint32_t)acc[j] == t[j];
            const unsigned long long blt = __ballot(lt), beq = __ballot(eq);
            const uint32_t slot = countsel_slot(lt, eq, blt, beq, run + 2 * j, wcnt + j * 8, wave, lower, below[j], need[j], a.k);
            if (slot != COUNTSEL_NO_SLOT) a.keys[(int64_t)(q0 + j) * a.k + slot] = ((uint64_t)(uint32_t)acc[j] << 32) | pos;
        }
        __syncthreads();
        if (tid < QT * 2) {
            const int j = tid >> 1, h = tid & 1;
            run[tid] += wcnt[(j * 4 + 0) * 2 + h] + wcnt[(j * 4 + 1) * 2 + h] + wcnt[(j * 4 + 2) * 2 + h] + wcnt[(j * 4 + 3) * 2 + h];
        }
        // (the next tile's staging barriers order this update before the next use of run and wcnt)
    }
}

// ---- launch plumbing --------------------------------------------------------------------------------------------------
int bq_cw(int W) { return W <= 4 ? 4 : W <= 8 ? 8 : W <= 12 ? 12 : W <= 16 ? 16 : 8; }
// the tile and the queries, under a list the staged ids in front of them
size_t bq_tile_lds(int W, int cw, int qt, bool mapped = false)
{
    return ((mapped ? (size_t)BQ_IDS_WORDS : 0) + (size_t)BQ_ROWS * (cw + 1) + (size_t)qt * ((W + cw - 1) / cw) * cw) * 8;
}

// the query tile of a launch (pick_qt) within the LDS budget, lds_per_query being what the kernel adds to the tile per query
int bq_qt(int nq, int W, size_t lds_per_query, bool mapped)
{
    const int cw = bq_cw(W);
    return pick_qt(nq, [&](int qt) { return bq_tile_lds(W, cw, qt, mapped) + (size_t)qt * lds_per_query <= BQ_LDS_BUDGET; });
}
// the widest single-query request: W = 128 (chunks of 8) with its histogram, under a list
static_assert(((size_t)BQ_IDS_WORDS + BQ_ROWS * 9 + 128) * 8 + (64 * 128 + 1) * 4 <= BQ_LDS_BUDGET, "one query always fits");

template <class F> void bq_with_cw(int cw, F &&f)
{
    switch (cw) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 12: f(std::integral_constant<int, 12>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
    }
}

// f(CW, QT, MAPPED) as integral constants
template <class F> void bq_with_form(int cw, int qt, bool mapped, F &&f)
{
    bq_with_cw(cw, [&](auto c) {
        with_qt(qt, [&](auto q) {
            if (mapped) f(c, q, std::true_type{});
            else f(c, q, std::false_type{});
        });
    });
}

} // namespace

void launch_bq_encode(const float *X, int64_t n, int dims, uint64_t *codes, hipStream_t s)
{
    if (n <= 0) return;
    const int W = (dims + 63) / 64;
    bq_encode_kernel<<<dim3((unsigned)grid_cap((n * W + 3) / 4, 1 << 20)), dim3(256), 0, s>>>(reinterpret_cast<const uint32_t *>(X), n, dims, W,
                                                                                            codes);
}

void launch_bq_decode(const uint64_t *codes, int64_t n, int dims, float *out, hipStream_t s)
{
    if (n <= 0) return;
    const int W = (dims + 63) / 64;
    bq_decode_kernel<<<dim3((unsigned)grid_cap((n * dims + 255) / 256, 1 << 20)), dim3(256), 0, s>>>(codes, n, dims, W, out);
}

void launch_bq_batch(const uint64_t *codes, int W, const uint64_t *qcode, int64_t row0, int64_t n, int32_t *out, hipStream_t s)
{
    if (n <= 0) return;
    const int cw = bq_cw(W);
    const BqRows rows{codes, W, row0 + n, nullptr};
    const unsigned grid = (unsigned)grid_cap((n + BQ_ROWS - 1) / BQ_ROWS, 1 << 16);
    bq_with_cw(cw, [&](auto c) {
        bq_batch_kernel<decltype(c)::value><<<dim3(grid), dim3(BQ_ROWS), bq_tile_lds(W, cw, 1), s>>>(rows, qcode, row0, n, out);
    });
}

void launch_bq_rerank(const uint64_t *codes, int W, int dims, int64_t ntotal, const uint64_t *qcode, const int64_t *rows, int64_t n,
                      float *dist, float *score, hipStream_t s)
{
    if (n <= 0) return;
    const int cw = bq_cw(W);
    const BqRows r{codes, W, ntotal, rows};
    const unsigned grid = (unsigned)grid_cap((n + BQ_ROWS - 1) / BQ_ROWS, 1 << 16);
    bq_with_cw(cw, [&](auto c) {
        bq_rerank_kernel<decltype(c)::value><<<dim3(grid), dim3(BQ_ROWS), bq_tile_lds(W, cw, 1), s>>>(r, qcode, n, dims, dist, score);
    });
}

void launch_bq_hist(const BqSearch &a, hipStream_t s)
{
    const bool mapped = a.rowmap != nullptr;
    const int cw = bq_cw(a.W), qt = bq_qt(a.nq, a.W, (size_t)(64 * a.W + 1) * 4, mapped);
    const size_t lds = bq_tile_lds(a.W, cw, qt, mapped) + (size_t)qt * (64 * a.W + 1) * 4;
    const dim3 grid((unsigned)a.nblk, (unsigned)((a.nq + qt - 1) / qt));
    bq_with_form(cw, qt, mapped, [&](auto c, auto q, auto m) {
        bq_hist_kernel<decltype(c)::value, decltype(q)::value, decltype(m)::value><<<grid, dim3(BQ_ROWS), lds, s>>>(a);
    });
}

void launch_bq_thresh(const BqSearch &a, hipStream_t s) { bq_thresh_kernel<<<dim3((unsigned)a.nq), dim3(256), 0, s>>>(a); }

void launch_bq_count(const BqSearch &a, hipStream_t s)
{
    const bool mapped = a.rowmap != nullptr;
    const int cw = bq_cw(a.W), qt = bq_qt(a.nq, a.W, 8, mapped);
    const size_t lds = bq_tile_lds(a.W, cw, qt, mapped) + (size_t)qt * 8;
    const dim3 grid((unsigned)a.nblk, (unsigned)((a.nq + qt - 1) / qt));
    bq_with_form(cw, qt, mapped, [&](auto c, auto q, auto m) {
        bq_count_kernel<decltype(c)::value, decltype(q)::value, decltype(m)::value><<<grid, dim3(BQ_ROWS), lds, s>>>(a);
    });
}

void launch_bq_emit(const BqSearch &a, hipStream_t s)
{
    const bool mapped = a.rowmap != nullptr;
    const int cw = bq_cw(a.W), qt = bq_qt(a.nq, a.W, 40, mapped);
    const size_t lds = bq_tile_lds(a.W, cw, qt, mapped) + (size_t)qt * 40;
    const dim3 grid((unsigned)a.nblk, (unsigned)((a.nq + qt - 1) / qt));
    bq_with_form(cw, qt, mapped, [&](auto c, auto q, auto m) {
        bq_emit_kernel<decltype(c)::value, decltype(q)::value, decltype(m)::value><<<grid, dim3(BQ_ROWS), lds, s>>>(a);
    });
}

} // namespace lb
