// kernels_gemm_tall2.hip -- candidate generation on the split-bf16 contraction, 256 rows x 256 queries per workgroup,
// whole 128-B lines per row and K-step.
//
// Contract: S = X_tile . Q_tile^T as hi*hi + hi*lo + lo*hi on
// v_mfma_f32_32x32x16_bf16, metric key and admission test fused into the epilogue; ranking semantics of
// BruteForceIndex.SearchVectors (internal/store/adaptive_index.go:161-225), per-pair arithmetic of the *Batch functions
// (internal/simd/batch_operations.go:64-157) approximated for the CANDIDATE keys only (the reported distances come from the
// exact re-rank).
//
// Why this shape.  The 256 x 128 tile of rounds 2-3 (removed in round 4) staged 64 B per row and K-step of 16: HALF a cache line.  The other half of the
// line is wanted one K-step later, by which time the CU's 32 KB vector L1 has turned over, so every line crosses the
// L2 -> L1 -> LDS path twice (and, measured with rocprofv3, reaches the fabric 1.99 times per algorithmic byte).  At
// 1024 queries the kernel asked its L2 for 8.8 TB/s of 64-B pieces -- half of what the same path delivers in whole lines
// (16.8-18.8 TB/s, MI355X_MICROARCH.md "Indexed rows: gather into LDS") -- and the matrix pipe sat at 53-60 % busy waiting
// for them (SQ_WAIT_ANY 38 % of the wave cycles, profiles/r02_pmc_sq_tall.txt).  Here a K-step is 32 floats = one 128-B line
// per row, a stage is 512 lines (64 KB: 256 corpus rows + 256 query rows), and 256 x 256 x 32 x 3 products are done per
// stage: 0.67 staged bytes per 1000 bf16 flop against 1.0 for the 256 x 128 tile, none of them fetched twice.
//
// Shape.  8 waves as 4 (rows) x 2 (queries); a wave owns 64 rows x 128 queries = 2 x 4 MFMA tiles (128 accumulator
// registers).  With the corpus operand split in registers (ASPLIT == 2) each 32-row fragment is split by the TWO waves that
// share it, not by four as a 128 x 64 wave tile in this workgroup would have it: 2 conversion instructions per MFMA instead
// of 4 (the matrix pipe leaves ~6 vector issue slots per 32x32x16 MFMA to ONE wave, and two waves share a SIMD).
// One workgroup per CU (2 x 64 KB ring + side inputs), one s_barrier per K-step of 32 = per 48 MFMAs of every wave; the DMA
// of stage k+1 is issued right behind the barrier that frees its slot and has the whole step (>= 3072 matrix-pipe cycles per
// SIMD) to land.
//
// Operands as in the first tall kernel: queries always as the split image (launch_split_bf16), the corpus as the same kind
// of image (ASPLIT == 1) or as plain f32 rows split in registers after the LDS read (ASPLIT == 2).
// Image layout (kernels_gemm.hip: split_bf16_kernel): per row and group of 16 k, 32 B of hi then 32 B of lo.
// Candidate keys, thresholds, the tile's side inputs, the admission rule and the workgroup-local list: lb_admit.h.
#include "lb_admit.h"

#include <type_traits>

namespace lb {

namespace {

constexpr int W_BM = 256, W_BN = 256, W_BK = 32; // tile rows, tile queries, floats per row and stage
constexpr int W_THREADS = 512;
constexpr int W_STAGE_F = (W_BM + W_BN) * W_BK; // floats per stage (64 KB)
constexpr int W_NST = 2;
constexpr int W_NI = 8; // DMA instructions per wave and stage: 4 x 8 corpus rows + 4 x 8 query rows

struct Tall2Args {
    const float *X;
    const float *norm2;
    const float *rnorm;
    int64_t row_begin, row_end;
    int D;
    const float *Q; // split image of the query batch
    int nq;
    const uint8_t *mask;
    const uint32_t *rowmap;
    CandState cs;
    int n_row_tiles, n_q_tiles;
    int boot;
};

// 128-B rows, eight 16-B chunks: chunk c of row r sits at position c ^ ((r >> 1) & 7), which spreads the 16 lanes of every
// ds_read_b128 group (16 rows that are distinct mod 16, same chunk) over all 64 banks
__device__ __forceinline__ int wswz(int row, int chunk) { return row * W_BK + ((chunk ^ ((row >> 1) & 7)) << 2); }

// Tried on this kernel and dropped:
//  * the next stage's requests spread between the MFMAs of the step (two behind every 6 or 12 MFMAs): any inline-asm
//    statement inside the unrolled MFMA block makes hipcc (ROCm 7.2) spill 130-230 registers -- and so do a wave-dependent
//    branch around the requests and two copies of the loop (the accumulator arrays are then not promoted to registers);
//  * an L2 prefetch of the stage after next by a plain global_load_dword into a register nobody reads: the load lands after
//    the asm statement has ended, the allocator has re-used the register by then and a pointer got overwritten (wrong
//    candidates and a memory fault).  An in-flight load needs a destination the compiler cannot touch.
template <int METRIC, int ASPLIT>
__global__ __launch_bounds__(W_THREADS, 2) void gemm_filter_tall2_kernel(Tall2Args a)
{
    // XCD-aware order as in gemm_filter_kernel: the query tiles of one corpus tile run side by side on one XCD
    const int b = blockIdx.x;
    const int xcd = b & 7;
    const int in_xcd = b >> 3;
    const int qt = in_xcd % a.n_q_tiles;
    const int rt = (in_xcd / a.n_q_tiles) * 8 + xcd;
    if (rt >= a.n_row_tiles) return;

    extern __shared__ __attribute__((aligned(16))) float wlds[];
    float *ring = wlds;                                              // [W_NST][A 256x32 | B 256x32]
    float *s_aux = ring + W_NST * W_STAGE_F;                         // [W_BM]
    uint32_t *s_rowid = reinterpret_cast<uint32_t *>(s_aux + W_BM);  // [W_BM]
    uint8_t *s_vis = reinterpret_cast<uint8_t *>(s_rowid + W_BM);    // [W_BM]
    const uint32_t ring_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float *)ring;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1; // 4 x 2 waves: rows 64 wr .. +63, queries 128 wc .. +127
    const int l31 = lane & 31, h = lane >> 5;
    const int64_t row0 = a.row_begin + (int64_t)rt * W_BM;
    const int q0 = qt * W_BN;
    const int64_t last_row = a.row_end - 1;
    const int last_q = a.nq - 1;

    auto corpus_row = [&](int64_t pos) -> int64_t {
        if (pos > last_row) pos = last_row;
        return a.rowmap ? (int64_t)a.rowmap[pos] : pos;
    };
    const int64_t side_ri = corpus_row(row0 + (tid & (W_BM - 1))); // threads 0 .. W_BM-1 carry one side input each

    // DMA sources.  A request fills 8 rows (1 KiB): lane l lands at (row l / 8, chunk POSITION l % 8) and therefore fetches
    // the chunk that belongs there: position ^ ((row >> 1) & 7).
    // Every wave requests its 32 corpus rows + 32 query rows (8 requests per stage).
    constexpr int NI = W_NI;
    constexpr int RPW = 32; // rows of each operand a wave stages
    const float *src[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int row = wave * RPW + (i % (NI / 2)) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        if (i < NI / 2) {
            src[i] = a.X + corpus_row(row0 + row) * (int64_t)a.D + 4 * c;
        } else {
            int qr = q0 + row;
            if (qr > last_q) qr = last_q;
            src[i] = a.Q + (int64_t)qr * a.D + 4 * c;
        }
    }
    // grouped requests: the instruction offset (i & 3) KiB also moves the global address
#pragma unroll
    for (int i = 0; i < NI; i++) src[i] -= (i & 3) * 256;
    auto issue = [&](int kt) {
        const uint32_t A = ring_base + (uint32_t)(kt & 1) * (W_STAGE_F * 4);
        const uint32_t B = A + W_BM * W_BK * 4;
        const int k0 = kt * W_BK;
        lds_dma16x4<false>(src[0] + k0, src[1] + k0, src[2] + k0, src[3] + k0, A + (uint32_t)(wave * RPW * W_BK * 4));
        lds_dma16x4<false>(src[4] + k0, src[5] + k0, src[6] + k0, src[7] + k0, B + (uint32_t)(wave * RPW * W_BK * 4));
    };

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int nk = a.D / W_BK; // D % 32 == 0 (launcher)
    issue(0);
    // one burst behind the first stage (not needed before the epilogue): side inputs and thresholds
    const float aux_r = side_aux<METRIC>(a.norm2, a.rnorm, side_ri);
    uint8_t side_vis = 1;
    if (a.mask) side_vis = a.mask[side_ri];
    float tk[4];
    uint32_t tr[4];
#pragma unroll
    for (int tn = 0; tn < 4; tn++) {
        const int qj = q0 + wc * 128 + tn * 32 + l31;
        const uint64_t tau = lane_tau(a.cs.tau, qj, a.nq, a.boot);
        tk[tn] = tau_key_of(tau);
        tr[tn] = entry_row(tau);
    }
    if (tid < W_BM) {
        s_aux[tid] = aux_r;
        s_vis[tid] = (row0 + tid <= last_row && side_vis) ? (uint8_t)1 : (uint8_t)0;
        s_rowid[tid] = (uint32_t)side_ri;
    }

    // one K-step; MORE (compile time): there is a next stage to request
    auto step = [&](int kt, auto more_tag) {
        constexpr bool MORE = decltype(more_tag)::value;
        wait_vmcnt<0>();                 // this wave's part of stage kt has landed (issued one whole K-step ago)
        __builtin_amdgcn_s_barrier(); // everyone's part is in; everyone is done reading stage kt - 1 (and, at kt = 0, has
                                      // written its side inputs)
        asm volatile("" ::: "memory");
        if (MORE) issue(kt + 1); // stage kt + 1 goes into the slot read at step kt - 1
        const float *As = ring + (kt & 1) * W_STAGE_F;
        const float *Bs = As + W_BM * W_BK;
        // The stage's two MFMA k-blocks of 16.  Per k-block: both corpus fragments (split once, used by all four query
        // tiles), then the query fragments one tile at a time (16 + 8 fragment registers live instead of 8 + 32).  The
        // second k-block's corpus fragments are fetched and split BEHIND the first query tile of the first k-block, so
        // that their ~50 conversion instructions issue between that k-block's MFMAs (which leave three quarters of the
        // vector issue slots free) instead of in front of the second k-block, where both waves of the SIMD would sit
        // through them at the same time.
        bf16x8 ah[2][2], al[2][2];
        auto load_a = [&](int kb) {
#pragma unroll
            for (int tm = 0; tm < 2; tm++) {
                const int r = wr * 64 + tm * 32 + l31;
                if (ASPLIT == 1) {
                    ah[kb][tm] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4 *>(&As[wswz(r, 4 * kb + h)]));
                    al[kb][tm] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4 *>(&As[wswz(r, 4 * kb + 2 + h)]));
                } else {
                    const f32x4 x0 = *reinterpret_cast<const f32x4 *>(&As[wswz(r, 4 * kb + 2 * h)]);
                    const f32x4 x1 = *reinterpret_cast<const f32x4 *>(&As[wswz(r, 4 * kb + 2 * h + 1)]);
                    split_bf16x8(x0, x1, ah[kb][tm], al[kb][tm]);
                }
            }
        };
        load_a(0);
#pragma unroll
        for (int kb = 0; kb < 2; kb++) {
#pragma unroll
            for (int tn = 0; tn < 4; tn++) {
                const int r = wc * 128 + tn * 32 + l31;
                const bf16x8 bh = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4 *>(&Bs[wswz(r, 4 * kb + h)]));
                const bf16x8 bl = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4 *>(&Bs[wswz(r, 4 * kb + 2 + h)]));
#pragma unroll
                for (int tm = 0; tm < 2; tm++) {
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[kb][tm], bh, acc[tm][tn], 0, 0, 0);
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kb][tm], bl, acc[tm][tn], 0, 0, 0);
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kb][tm], bh, acc[tm][tn], 0, 0, 0);
                }
                if (kb == 0 && tn == 0) load_a(1);
            }
        }
    };
    for (int kt = 0; kt + 1 < nk; kt++) step(kt, std::true_type{});
    step(nk - 1, std::false_type{});

    // ---- epilogue: key + admission, one MFMA row tile (this lane's 16 rows of it) at a time ----------------
    // C layout (32x32): col = lane & 31 (query), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
    // workgroup-local admission list, carved from the ring (free: every wave is past the last K-step's reads once the
    // barrier below is behind it)
    const LocalList<4096, W_BN, W_THREADS> fl(reinterpret_cast<uint32_t *>(ring), reinterpret_cast<uint64_t *>(ring + 1024));
    __syncthreads();
    fl.reset(tid);
    __syncthreads();
#pragma unroll
    for (int tm = 0; tm < 2; tm++) {
        float aux[4][4];
        uint32_t rid[4][4];
        uint32_t vbits = 0; // bit (g*4 + e): row visible (in range and not masked out)
#pragma unroll
        for (int g = 0; g < 4; g++) // 4 consecutive local rows
            vbits |= tile_rows4(s_aux, s_rowid, s_vis, wr * 64 + tm * 32 + 8 * g + 4 * h, aux[g], rid[g]) << (g * 4);
#pragma unroll
        for (int tn = 0; tn < 4; tn++) {
            const int qj = q0 + wc * 128 + tn * 32 + l31;
            const bool qok = qj < a.nq;
            uint64_t *list = a.cs.lists + (size_t)(qok ? qj : 0) * a.cs.cap;
            if (a.boot) { // sample pass: the entry of position p goes to list[p - row_begin]
                if (qok) {
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const int64_t rbase = row0 + wr * 64 + tm * 32 + 8 * g + 4 * h;
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            if (rbase + e < a.row_end)
                                list[rbase + e - a.row_begin] = ((vbits >> (g * 4 + e)) & 1u) ? pack_entry(cand_key<METRIC>(acc[tm][tn][4 * g + e], aux[g][e]), rid[g][e])
                                                                                : kEntryMax;
                    }
                }
                continue;
            }
            // exact rule (lb_admit.h; a padded query's tau decodes to NaN)
            uint32_t bits = 0;
#pragma unroll
            for (int g = 0; g < 4; g++)
#pragma unroll
                for (int e = 0; e < 4; e++)
                    bits |= admit_exact(cand_key<METRIC>(acc[tm][tn][4 * g + e], aux[g][e]), rid[g][e], tk[tn], tr[tn]) << (g * 4 + e);
            bits &= vbits;
            if (bits) {
                const uint32_t n = (uint32_t)__builtin_popcount(bits);
                uint32_t lp = atomicAdd(fl.cnt, n);
                if (lp + n <= (uint32_t)fl.CAP) {
                    uint32_t lr = atomicAdd(&fl.qcnt[qj - q0], n);
#pragma unroll
                    for (int g = 0; g < 4; g++)
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            if (bits & (1u << (g * 4 + e))) {
                                fl.ent[lp] = pack_entry(cand_key<METRIC>(acc[tm][tn][4 * g + e], aux[g][e]), rid[g][e]);
                                fl.q[lp] = (uint16_t)(qj - q0);
                                fl.rk[lp] = (uint16_t)lr;
                                lp++;
                                lr++;
                            }
                    bits = 0; // done
                } else {
                    fl.reserved_unused(lp, n);
                }
            }
            if (bits) { // (local list full) one returning atomic reserves the lane's slots; the stores are fire-and-forget
                uint32_t pos = atomicAdd(&a.cs.cnt[qj], (uint32_t)__builtin_popcount(bits));
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (bits & (1u << (g * 4 + e))) {
                            if (pos < a.cs.cap) list[pos] = pack_entry(cand_key<METRIC>(acc[tm][tn][4 * g + e], aux[g][e]), rid[g][e]);
                            pos++;
                        }
            }
        }
    }
    if (!a.boot) fl.flush(tid, a.cs, q0);
}

} // namespace

// Requires D % 32 == 0, 16-B aligned X / Q; Q is the split image of the batch; asplit: 1 = X is the split image of
// the corpus, 2 = X is the plain f32 corpus.
void launch_gemm_filter_tall2(int metric, const float *X, const float *norm2, const float *rnorm, int64_t row_begin,
                              int64_t row_end, int D, const float *Qs, int nq, const uint8_t *mask, const uint32_t *rowmap,
                              CandState cs, bool boot, int asplit, hipStream_t s)
{
    if (row_end <= row_begin || nq <= 0) return;
    Tall2Args a;
    a.rowmap = rowmap;
    a.X = X; a.norm2 = norm2; a.rnorm = rnorm; a.row_begin = row_begin; a.row_end = row_end; a.D = D;
    a.Q = Qs; a.nq = nq; a.mask = mask; a.cs = cs; a.boot = boot ? 1 : 0;
    a.n_row_tiles = (int)((row_end - row_begin + W_BM - 1) / W_BM);
    a.n_q_tiles = (nq + W_BN - 1) / W_BN;
    const int groups = (a.n_row_tiles + 7) / 8;
    dim3 grid((unsigned)(groups * 8 * a.n_q_tiles));
    const size_t shmem = (size_t)W_NST * W_STAGE_F * 4 + W_BM * 4 + W_BM * 4 + W_BM;
#define LB_TALL2(M, SP)                                                                                             \
    do {                                                                                                            \
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_filter_tall2_kernel<M, SP>),                 \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem); /* per device */         \
        hipLaunchKernelGGL((gemm_filter_tall2_kernel<M, SP>), grid, dim3(W_THREADS), shmem, s, a);                  \
    } while (0)
#define LB_TALL2_M(M)                    \
    do {                                 \
        if (asplit == 1) LB_TALL2(M, 1); \
        else LB_TALL2(M, 2);             \
    } while (0)
    if (metric == METRIC_L2) LB_TALL2_M(METRIC_L2);
    else if (metric == METRIC_COS) LB_TALL2_M(METRIC_COS);
    else LB_TALL2_M(METRIC_DOT);
#undef LB_TALL2_M
#undef LB_TALL2
}

} // namespace lb
