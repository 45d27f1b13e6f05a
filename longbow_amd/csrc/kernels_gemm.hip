// kernels_gemm.hip -- candidate generation for batched k-NN on gfx950.
//
// The one dense contraction of the path: S = X_tile . Q_tile^T on the f32 MFMA
// (v_mfma_f32_32x32x2_f32, exact f32 fma chain), with the metric key and the
// top-k admission test fused into the epilogue so the nq x N score matrix never
// reaches HBM.  Replaces the per-pair loops of simd.EuclideanDistanceBatchFlat /
// CosineDistanceBatch / DotProductBatch (internal/simd/batch_operations.go:64-157)
// when many queries are in flight; ranking semantics of
// BruteForceIndex.SearchVectors (internal/store/adaptive_index.go:161-225).
//
// Tile: 128 corpus rows x 128 queries per workgroup, BK = 32 floats (one 128-B
// line per row per step), 4 waves (2x2), each wave 64x64 = 2x2 MFMA 32x32 tiles.
// LDS: [128][32] f32 per operand per stage, 16-B chunks XOR-swizzled by
// (row>>1)&7 so the ds_read_b128 fragment reads are bank-conflict free.
// Large non-boot passes with D % 32 == 0 and 16-B rows run a second body of the same contraction,
// gemm_filter_wide256_kernel below: 256 rows x 128 queries per workgroup on a ring of three 16-k
// stages, same k order per accumulator, bit-identical keys (selection: launch_gemm_filter).
// Candidate keys, thresholds, the tile's side inputs and the admission rule: lb_admit.h.
#include "lb_admit.h"

#include <atomic>
#include <cstdlib>

namespace lb {

constexpr int BM = 128; // corpus rows per tile (MFMA A operand, output rows)
constexpr int BN = 128; // queries per tile   (MFMA B operand, output cols = lanes)
constexpr int BK = 32;
constexpr int GEMM_THREADS = 256;

struct GemmArgs {
    const float *X;
    const float *norm2;
    const float *rnorm;
    int64_t row_begin, row_end;
    int D;
    const float *Q;
    int nq;
    const uint8_t *mask;
    const uint32_t *rowmap; // filtered search over a compacted row list: position -> corpus row (or null)
    CandState cs;
    int n_row_tiles, n_q_tiles;
    int boot; // bootstrap chunk: store every row at list[row - row_begin], no test, no atomics
};

__device__ __forceinline__ int swz_off(int row, int chunk)
{
    return row * BK + ((chunk ^ ((row >> 1) & 7)) << 2);
}

// MODE 2: D % 32 == 0 and 16-B aligned rows -> unconditional 16-B loads
// MODE 1: D % 4 == 0 and aligned -> 16-B loads, chunks past D read as zero
// MODE 0: anything else -> guarded scalar loads
template <int MODE>
__device__ __forceinline__ f32x4 load_chunk(const float *base, int64_t row, int D, int k)
{
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const float *p = base + row * (int64_t)D + k;
    if (MODE == 2) {
        v = *reinterpret_cast<const f32x4 *>(p);
    } else if (MODE == 1) {
        if (k < D) v = *reinterpret_cast<const f32x4 *>(p);
    } else {
        if (k + 0 < D) v.x = p[0];
        if (k + 1 < D) v.y = p[1];
        if (k + 2 < D) v.z = p[2];
        if (k + 3 < D) v.w = p[3];
    }
    return v;
}

// ALIGNED == 2 (GLDS): stage tiles with direct-to-LDS DMA loads (global_load_lds_dwordx4); the other modes stage through registers.
// The LDS image is lane-linear per wave instruction (base + lane*16), so the chunk swizzle is
// applied to the per-lane SOURCE address; the image is identical to the register-staged one.
template <int METRIC, int ALIGNED>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_filter_kernel(GemmArgs a)
{
    constexpr bool GLDS = ALIGNED == 2;
    // XCD-aware tile order: blocks b and b+8 share an XCD (round-robin dispatch), so the
    // n_q_tiles query tiles of one corpus tile are issued back-to-back on ONE XCD and the
    // corpus tile is pulled from HBM into that XCD's L2 once.  Placement only affects speed.
    const int b = blockIdx.x;
    const int xcd = b & 7;
    const int in_xcd = b >> 3;
    const int qt = in_xcd % a.n_q_tiles;
    const int rt = (in_xcd / a.n_q_tiles) * 8 + xcd;
    if (rt >= a.n_row_tiles) return;

    // one LDS object: [stage][A|B][BM*BK] f32 tiles, then the tile's per-row side inputs
    // (norm / 1/norm and the predicate byte), fetched once at kernel entry
    __shared__ __attribute__((aligned(16))) float lds_all[2 * 2 * BM * BK + BM + BM + BM / 4];
    float(*lds)[2][BM * BK] = reinterpret_cast<float(*)[2][BM * BK]>(lds_all);
    float *s_aux = lds_all + 2 * 2 * BM * BK;
    uint32_t *s_rowid = reinterpret_cast<uint32_t *>(s_aux + BM); // corpus row of each tile row
    uint8_t *s_vis = reinterpret_cast<uint8_t *>(s_rowid + BM);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, h = lane >> 5;

    const int64_t row0 = a.row_begin + (int64_t)rt * BM;
    const int q0 = qt * BN;
    const int64_t last_row = a.row_end - 1;
    const int last_q = a.nq - 1;

    auto corpus_row = [&](int64_t pos) -> int64_t { // positions index the (possibly compacted) row list
        if (pos > last_row) pos = last_row;
        return a.rowmap ? (int64_t)a.rowmap[pos] : pos;
    };
    // (the tile's side inputs and thresholds are fetched AFTER the first stage's DMA has been issued, see
    // below: they are not needed before the epilogue and would otherwise put two to three serial memory
    // round trips in front of the first K-step)
    const int64_t side_ri = corpus_row(row0 + (tid & (BM - 1)));

    // staging assignment: 4 chunks of 16 B per operand per thread
    int st_row[4], st_ch[4];
    int64_t st_xrow[4];
    int st_qrow[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int c = tid + GEMM_THREADS * i;
        st_row[i] = c >> 3;
        st_ch[i] = c & 7;
        st_xrow[i] = corpus_row(row0 + st_row[i]);
        int qr = q0 + st_row[i];
        st_qrow[i] = qr < last_q ? qr : last_q;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int nk = (a.D + BK - 1) / BK;
    f32x4 ra[4], rb[4];

    // GLDS staging: wave w issues instructions 4w..4w+3 per operand; instruction j fills LDS rows
    // 8j..8j+7 (1 KiB); lane l lands at (row 8j + l/8, chunk position l%8) and therefore fetches
    // source chunk (l%8) ^ ((row>>1)&7) of that row.
    const float *gsrcA[4], *gsrcB[4];
    if (GLDS) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int j = wave * 4 + i;
            const int row = j * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            const int64_t xr = corpus_row(row0 + row);
            int qr = q0 + row;
            if (qr > last_q) qr = last_q;
            gsrcA[i] = a.X + xr * (int64_t)a.D + 4 * c;
            gsrcB[i] = a.Q + (int64_t)qr * a.D + 4 * c;
        }
    }
    // one staging piece p = 0..7 (A0 B0 A1 B1 .. A3 B3).  The LDS destination is built from a wave index the compiler
    // can see is uniform, so m0 is scalar arithmetic (no v_readfirstlane per piece): a piece costs one 64-bit address
    // add on top of its global_load_lds.
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto glds_piece = [&](int p, int stage, int k0) {
        const int i = p >> 1;
        const int j = wave_u * 4 + i;
        if ((p & 1) == 0)
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)(gsrcA[i] + k0),
                (__attribute__((address_space(3))) void *)(&lds[stage][0][j * 8 * BK]), 16, 0,
                2); // aux 2 = nt: the corpus streams through once; keeps Q resident in L2
                    // (measured: L2-miss traffic 2.5x -> 1.8x algorithmic, same speed)
        else
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)(gsrcB[i] + k0),
                (__attribute__((address_space(3))) void *)(&lds[stage][1][j * 8 * BK]), 16, 0, 0);
    };
    auto glds_stage = [&](int stage, int k0) {
#pragma unroll
        for (int p = 0; p < 8; p++) glds_piece(p, stage, k0);
    };
    // prologue: stage 0
    if (GLDS) glds_stage(0, 0);
    // one burst behind the DMA: side inputs of tile row (tid & 127) and this lane's two thresholds; nothing
    // is consumed before every load has been issued
    const float aux_r = side_aux<METRIC>(a.norm2, a.rnorm, side_ri);
    uint8_t side_vis = 1;
    if (a.mask) side_vis = a.mask[side_ri];
    uint64_t tau_raw[2];
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        const int qj = q0 + wc * 64 + tn * 32 + l31;
        tau_raw[tn] = lane_tau(a.cs.tau, qj, a.nq, a.boot);
    }
    if (tid < BM) {
        s_aux[tid] = aux_r;
        s_vis[tid] = (row0 + tid <= last_row && side_vis) ? (uint8_t)1 : (uint8_t)0;
        s_rowid[tid] = (uint32_t)side_ri;
    }
    // admission thresholds of this lane's two queries, split into (key, row)
    float tau_key[2];
    uint32_t tau_row[2];
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        tau_key[tn] = tau_key_of(tau_raw[tn]);
        tau_row[tn] = entry_row(tau_raw[tn]);
    }
    if (!GLDS) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            ra[i] = load_chunk<ALIGNED>(a.X, st_xrow[i], a.D, st_ch[i] * 4);
            rb[i] = load_chunk<ALIGNED>(a.Q, st_qrow[i], a.D, st_ch[i] * 4);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            *reinterpret_cast<f32x4 *>(&lds[0][0][swz_off(st_row[i], st_ch[i])]) = ra[i];
            *reinterpret_cast<f32x4 *>(&lds[0][1][swz_off(st_row[i], st_ch[i])]) = rb[i];
        }
    }
    __syncthreads();

    if constexpr (GLDS) {
        // Main loop of the f32 GLDS tile, rotated by one sub-step so that no LDS or DMA issue sits outside the
        // MFMA stream.  A K-step is 4 sub-steps of 16 MFMAs (2 k per MFMA, lane halves on alternate 16-B chunks).
        // Two named fragment sets alternate: F0 feeds sub-steps 0 and 2, F1 sub-steps 1 and 3, and the reads of
        // sub-step s+1 are issued after the first 2 of sub-step s's MFMAs, 14 MFMAs before their use.  (hipcc waits
        // for them with lgkmcnt(0), which also waits for every younger read: reads issued ahead of those 2 MFMAs
        // would be waited for in full before the sub-step could start.)  The barrier closes
        // sub-step 2 (the last reads of the stage and the next stage's DMA have landed); sub-step 3 runs after it,
        // together with the next K-step's sub-step-0 reads and the DMA of the stage after that into the buffer
        // the barrier has just released.  Every accumulator sees the same k order as in the register-staged loop.
        struct Frag {
            f32x4 a[2], b[2];
        };
        auto ldfrag = [&](Frag &f, int stage, int s) {
            const float *As = lds[stage][0];
            const float *Bs = lds[stage][1];
            const int ch = 2 * s + h; // the two lane halves take alternate 16-B chunks (same k permutation for A and B)
#pragma unroll
            for (int t = 0; t < 2; t++) {
                f.a[t] = *reinterpret_cast<const f32x4 *>(&As[swz_off(wr * 64 + t * 32 + l31, ch)]);
                f.b[t] = *reinterpret_cast<const f32x4 *>(&Bs[swz_off(wc * 64 + t * 32 + l31, ch)]);
            }
        };
        auto mfma16 = [&](const Frag &f) {
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int tm = 0; tm < 2; tm++)
#pragma unroll
                    for (int tn = 0; tn < 2; tn++)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[tm][e], f.b[tn][e], acc[tm][tn], 0, 0, 0);
        };
        Frag F0, F1;
        // sub-steps 0-2 of a K-step (F0 holds sub-step 0's fragments on entry, F1 holds sub-step 3's on exit)
        auto steps012 = [&](int cur) {
            ldfrag(F1, cur, 1);
            mfma16(F0);
            ldfrag(F0, cur, 2);
            mfma16(F1);
            ldfrag(F1, cur, 3);
            mfma16(F0);
#pragma unroll
            for (int s = 0; s < 3; s++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); // MFMA: sub-step s
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0); // DS_READ: sub-step s+1's fragments
                __builtin_amdgcn_sched_group_barrier(0x008, 14, 0); // MFMA: sub-step s
            }
            __builtin_amdgcn_sched_barrier(0); // sub-step 2's MFMAs stay in front of the barrier
        };
        ldfrag(F0, 0, 0);
        if (nk > 1) glds_stage(1, BK);
        int kt = 0;
        for (; kt + 2 < nk; kt++) {
            const int cur = kt & 1;
            steps012(cur);
            __syncthreads();
            // sub-step 3 + the next K-step's sub-step-0 reads + the 8 pieces of stage kt+2 (into the buffer the
            // barrier has just released), one piece after every other MFMA; the pieces land before the next barrier
            const int k0 = (kt + 2) * BK;
            ldfrag(F0, cur ^ 1, 0);
#pragma unroll
            for (int p = 0; p < 8; p++) glds_piece(p, cur, k0);
            mfma16(F1);
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0); // DS_READ
#pragma unroll
            for (int p = 0; p < 7; p++) {
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); // VMEM_READ (global_load_lds)
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); // MFMA
            }
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); // VMEM_READ
        }
        if (kt + 1 < nk) { // the last K-step but one: nothing left to stage
            const int cur = kt & 1;
            steps012(cur);
            __syncthreads();
            ldfrag(F0, cur ^ 1, 0);
            mfma16(F1);
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0); // DS_READ
            __builtin_amdgcn_sched_group_barrier(0x008, 14, 0); // MFMA
            kt++;
        }
        // the last K-step: no barrier, LDS is not written again
        steps012(kt & 1);
        mfma16(F1);
    } else {
        // Main loop of the register-staged tiles.  Per K-step (BK = 32): the next stage's global loads are
        // issued first, the fragment reads of sub-step s+1 are issued before the 16 MFMAs of sub-step s
        // (register double buffer), and the LDS write of the next stage happens in the middle of the MFMA
        // stream (its target buffer was released by the barrier that ended the previous K-step), so
        // the only serial section left at the end of a K-step is the barrier itself.
        for (int kt = 0; kt < nk; kt++) {
            const int cur = kt & 1;
            const bool has_next = kt + 1 < nk;
            if (has_next) {
                const int k0 = (kt + 1) * BK;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    ra[i] = load_chunk<ALIGNED>(a.X, st_xrow[i], a.D, k0 + st_ch[i] * 4);
                    rb[i] = load_chunk<ALIGNED>(a.Q, st_qrow[i], a.D, k0 + st_ch[i] * 4);
                }
            }
            const float *As = lds[cur][0];
            const float *Bs = lds[cur][1];
            f32x4 fa[2][2], fb[2][2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                fa[0][t] = *reinterpret_cast<const f32x4 *>(&As[swz_off(wr * 64 + t * 32 + l31, h)]);
                fb[0][t] = *reinterpret_cast<const f32x4 *>(&Bs[swz_off(wc * 64 + t * 32 + l31, h)]);
            }
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int cb = s & 1, nb = cb ^ 1;
                if (s < 3) {
                    const int ch = 2 * (s + 1) + h; // the two lane halves take alternate 16-B chunks;
                                                    // the same k permutation is applied to A and B.
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        fa[nb][t] = *reinterpret_cast<const f32x4 *>(&As[swz_off(wr * 64 + t * 32 + l31, ch)]);
                        fb[nb][t] = *reinterpret_cast<const f32x4 *>(&Bs[swz_off(wc * 64 + t * 32 + l31, ch)]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int tm = 0; tm < 2; tm++)
#pragma unroll
                        for (int tn = 0; tn < 2; tn++)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cb][tm][e], fb[cb][tn][e],
                                                                              acc[tm][tn], 0, 0, 0);
                if (s == 1 && has_next) {
                    const int nxt = cur ^ 1;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        *reinterpret_cast<f32x4 *>(&lds[nxt][0][swz_off(st_row[i], st_ch[i])]) = ra[i];
                        *reinterpret_cast<f32x4 *>(&lds[nxt][1][swz_off(st_row[i], st_ch[i])]) = rb[i];
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- epilogue: key + admission -------------------------------------------------
    // C layout (32x32): col = lane&31 (query), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
    // All per-row side inputs (norm / mask) are fetched up front in one burst: a load per
    // element inside the admission loop would serialise 64 L2 round trips per lane.
    float aux[2][4][4];
    uint32_t rid[2][4][4]; // corpus row ids of this lane's 32 rows
    uint32_t vbits = 0; // bit (tm*16 + g*4 + e): row visible (in range and not masked out)
#pragma unroll
    for (int tm = 0; tm < 2; tm++)
#pragma unroll
        for (int g = 0; g < 4; g++) // 4 consecutive local rows
            vbits |= tile_rows4(s_aux, s_rowid, s_vis, wr * 64 + tm * 32 + 8 * g + 4 * h, aux[tm][g], rid[tm][g]) << (tm * 16 + g * 4);
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        const int qj = q0 + wc * 64 + tn * 32 + l31;
        const bool qok = qj < a.nq;
        uint64_t *list = a.cs.lists + (size_t)(qok ? qj : 0) * a.cs.cap;
        if (a.boot) {
            // bootstrap chunk: entry of row r goes to list[r - row_begin]; a lane's 4 consecutive
            // rows are 32 contiguous bytes -> two 16-B stores
            if (qok) {
#pragma unroll
                for (int tm = 0; tm < 2; tm++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const int64_t rbase = row0 + wr * 64 + tm * 32 + 8 * g + 4 * h;
                        uint64_t ent[4];
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            ent[e] = ((vbits >> (tm * 16 + g * 4 + e)) & 1u) ? pack_entry(cand_key<METRIC>(acc[tm][tn][4 * g + e], aux[tm][g][e]), rid[tm][g][e]) : kEntryMax;
                        uint64_t *dst = list + (rbase - a.row_begin);
                        if (rbase + 3 < a.row_end) {
                            typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
                            u64x2 v0 = {ent[0], ent[1]}, v1 = {ent[2], ent[3]};
                            *reinterpret_cast<u64x2 *>(dst) = v0;
                            *reinterpret_cast<u64x2 *>(dst + 2) = v1;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; e++)
                                if (rbase + e < a.row_end) dst[e] = ent[e];
                        }
                    }
            }
            continue;
        }
        // pass 1 (branch-free): which of this lane's 32 elements pass the admission test (lb_admit.h:
        // exact rule; tau of an out-of-range query decodes to NaN, so nothing passes)
        uint32_t bits = 0;
#pragma unroll
        for (int tm = 0; tm < 2; tm++)
#pragma unroll
            for (int g = 0; g < 4; g++)
#pragma unroll
                for (int e = 0; e < 4; e++)
                    bits |= admit_exact(cand_key<METRIC>(acc[tm][tn][4 * g + e], aux[tm][g][e]), rid[tm][g][e], tau_key[tn], tau_row[tn]) << (tm * 16 + g * 4 + e);
        bits &= vbits;
        // ONE returning atomic per lane reserves the slots; the stores are fire-and-forget
        if (bits) {
            uint32_t pos = atomicAdd(&a.cs.cnt[qj], (uint32_t)__builtin_popcount(bits));
#pragma unroll
            for (int tm = 0; tm < 2; tm++)
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (bits & (1u << (tm * 16 + g * 4 + e))) {
                            const uint32_t ri = rid[tm][g][e];
                            if (pos < a.cs.cap) list[pos] = pack_entry(cand_key<METRIC>(acc[tm][tn][4 * g + e], aux[tm][g][e]), ri);
                            pos++;
                        }
        }
    }
}

// ---- the 256-row body of the f32 GLDS tile -------------------------------------------------------------------------------
// gemm_filter_wide256_kernel: 256 corpus rows x 128 queries per workgroup, 4 waves (2x2), each wave 128 rows x 64 queries =
// 4x2 MFMA 32x32 tiles (128 accumulator registers), two workgroups per CU.  Per product it stages three quarters of the
// 128-row tile's bytes and DMA pieces (24 KB per 256 x 128 x 16 against 32 KB per 128 x 128 x 32), issues 12 fragment
// reads per 64 MFMAs in place of 16, and pays prologue, epilogue and dispatch half as often.
// K-step: 16 floats (64 B per row), two sub-steps of 32 MFMAs; the lane halves take chunks 2s and 2s+1 of sub-step s, so
// every accumulator sees k in the order the 128-row tile gives it and the candidate keys are bit-identical.
// LDS: a ring of three stages [A 256x16 | B 128x16] f32 (24 KB each, 16-B chunks XOR-swizzled by (row>>2)&3 so that the
// 16 rows of a ds_read_b128 group cover all 64 banks), then the side inputs of the 256 rows: 76,032 B, twice per CU.
// Staging: direct-to-LDS DMA as inline asm with counted vmcnt waits -- with the builtin the compiler's wait pass puts
// vmcnt(0) in front of every later LDS read, which would wait for the stage that has just been requested.  Stage j+3 is
// requested behind the barrier of step j into the slot stage j was read from (its last fragments are in registers by then)
// and has to be in by the barrier of step j+2: two K-steps of prefetch.  Schedule as in the 128-row loop: the reads of the
// next sub-step sit behind the first 2 MFMAs of the current one, the 6 DMA pieces one per 4 MFMAs from the 8th MFMA behind
// the barrier on, the last three steps are peeled (nothing left to request; the last one has no barrier).
// Launched for non-boot passes only (launch_gemm_filter); D % 32 == 0, X and Q 16-B aligned.
constexpr int WBM = 256;                        // corpus rows per tile
constexpr int WBK = 16;                         // floats per K-step
constexpr int WNST = 3;                         // ring stages
constexpr int W_STAGE_F = (WBM + BN) * WBK;     // floats per stage
constexpr int W_NI = 6;                         // DMA instructions per wave and stage: 4 x 16 corpus rows + 2 x 16 query rows

// 64-B rows: the 16-B chunk of row r lands at position chunk ^ ((r >> 2) & 3)
__device__ __forceinline__ int wswz(int row, int chunk) { return row * WBK + ((chunk ^ ((row >> 2) & 3)) << 2); }

// 16 B per lane straight into LDS (lane l lands at lds_addr + 16 l).  NT: the corpus' cache policy, see kWide256CorpusNT.
template <bool NT>
__device__ __forceinline__ void wide_dma16(const void *gsrc, uint32_t lds_addr)
{
    uint32_t save;
    if (NT)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                     : "=&s"(save) : "v"(gsrc), "s"(lds_addr) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(save) : "v"(gsrc), "s"(lds_addr) : "memory");
}
// s_waitcnt vmcnt(VM) lgkmcnt(LGKM) (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] << 14)
template <int VM, int LGKM>
__device__ __forceinline__ void wide_wait()
{
    __builtin_amdgcn_s_waitcnt((VM & 15) | (7 << 4) | (LGKM << 8) | ((VM >> 4) << 14));
    asm volatile("" ::: "memory");
}
// A row's 128-B line is consumed over two K-steps, so it has to survive in L2 in between: default policy
// (nt measured level on the headline shape, LABNOTES R32.1).
constexpr bool kWide256CorpusNT = false;

// the barrier of a step: this wave's part of the next stage is in once only the VM requests behind it are outstanding,
// and its reads of the current stage have landed (that slot is requested into right behind the barrier)
template <int VM>
__device__ __forceinline__ void wide_step_barrier()
{
    wide_wait<VM, 0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

struct WideFrag {
    f32x4 a[4], b[2];
};
// MFMAs FROM .. TO-1 of a sub-step's 32: i -> element i / 8 of the chunk pair, row tile (i / 2) % 4, query tile i % 2
template <int FROM, int TO>
__device__ __forceinline__ void wide_mfma(f32x16 (&acc)[4][2], const WideFrag &f)
{
#pragma unroll
    for (int i = FROM; i < TO; i++) {
        const int e = i >> 3, tm = (i >> 1) & 3, tn = i & 1;
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[tm][e], f.b[tn][e], acc[tm][tn], 0, 0, 0);
    }
}

template <int METRIC>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_filter_wide256_kernel(GemmArgs a)
{
    // XCD-aware tile order as in gemm_filter_kernel
    const int b = blockIdx.x;
    const int xcd = b & 7;
    const int in_xcd = b >> 3;
    const int qt = in_xcd % a.n_q_tiles;
    const int rt = (in_xcd / a.n_q_tiles) * 8 + xcd;
    if (rt >= a.n_row_tiles) return;

    __shared__ __attribute__((aligned(16))) float lds_all[WNST * W_STAGE_F + WBM + WBM + WBM / 4];
    float *ring = lds_all; // [WNST][A 256x16 | B 128x16]
    float *s_aux = ring + WNST * W_STAGE_F;
    uint32_t *s_rowid = reinterpret_cast<uint32_t *>(s_aux + WBM);
    uint8_t *s_vis = reinterpret_cast<uint8_t *>(s_rowid + WBM);
    const uint32_t ring_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float *)ring;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, h = lane >> 5;

    const int64_t row0 = a.row_begin + (int64_t)rt * WBM;
    const int q0 = qt * BN;
    const int64_t last_row = a.row_end - 1;
    const int last_q = a.nq - 1;

    auto corpus_row = [&](int64_t pos) -> int64_t { // positions index the (possibly compacted) row list
        if (pos > last_row) pos = last_row;
        return a.rowmap ? (int64_t)a.rowmap[pos] : pos;
    };
    const int64_t side_ri = corpus_row(row0 + tid); // one side input per thread

    // DMA sources.  Instruction i of this wave fills 16 rows (1 KiB): corpus rows 64 wave + 16 i .. +15, query rows
    // 32 wave + 16 i .. +15; lane l lands at (row l / 4, chunk position l % 4) and fetches source chunk (l % 4) ^ ((row>>2)&3).
    const float *srcA[4], *srcB[2];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = wave * 64 + i * 16 + (lane >> 2);
        const int c = (lane & 3) ^ ((row >> 2) & 3);
        srcA[i] = a.X + corpus_row(row0 + row) * (int64_t)a.D + 4 * c;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int row = wave * 32 + i * 16 + (lane >> 2);
        const int c = (lane & 3) ^ ((row >> 2) & 3);
        int qr = q0 + row;
        if (qr > last_q) qr = last_q;
        srcB[i] = a.Q + (int64_t)qr * a.D + 4 * c;
    }
    // one staging piece p = 0..5 (A0 .. A3 B0 B1) of the stage at k0 into ring slot `slot`
    auto piece = [&](int p, int slot, int k0) {
        const uint32_t A = ring_base + (uint32_t)slot * (W_STAGE_F * 4);
        if (p < 4)
            wide_dma16<kWide256CorpusNT>(srcA[p] + k0, A + (uint32_t)((wave * 64 + p * 16) * WBK * 4));
        else
            wide_dma16<false>(srcB[p - 4] + k0, A + (uint32_t)(WBM * WBK * 4 + (wave * 32 + (p - 4) * 16) * WBK * 4));
    };
    auto issue = [&](int slot, int k0) {
#pragma unroll
        for (int p = 0; p < W_NI; p++) piece(p, slot, k0);
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int nk = a.D / WBK; // D % 32 == 0 (launcher): an even count, at least 2
    issue(0, 0);
    issue(1, WBK);
    if (nk > 2) issue(2, 2 * WBK);
    // one burst behind the first stages: side inputs of tile row tid and this lane's two thresholds
    const float aux_r = side_aux<METRIC>(a.norm2, a.rnorm, side_ri);
    uint8_t side_vis = 1;
    if (a.mask) side_vis = a.mask[side_ri];
    uint64_t tau_raw[2];
#pragma unroll
    for (int tn = 0; tn < 2; tn++) tau_raw[tn] = lane_tau(a.cs.tau, q0 + wc * 64 + tn * 32 + l31, a.nq, false);
    s_aux[tid] = aux_r;
    s_vis[tid] = (row0 + tid <= last_row && side_vis) ? (uint8_t)1 : (uint8_t)0;
    s_rowid[tid] = (uint32_t)side_ri;
    float tau_key[2];
    uint32_t tau_row[2];
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        tau_key[tn] = tau_key_of(tau_raw[tn]);
        tau_row[tn] = entry_row(tau_raw[tn]);
    }
    wide_wait<0, 0>(); // the stages requested and every load above (the compiler cannot count the DMA)
    __syncthreads();   // side inputs written (the loop below uses bare barriers: no LDS writes of its own)

    WideFrag F0, F1;
    auto ldfrag = [&](WideFrag &f, int slot, int s) {
        const float *As = ring + slot * W_STAGE_F;
        const float *Bs = As + WBM * WBK;
        const int ch = 2 * s + h; // the two lane halves take alternate 16-B chunks (same k permutation for A and B)
#pragma unroll
        for (int t = 0; t < 4; t++) f.a[t] = *reinterpret_cast<const f32x4 *>(&As[wswz(wr * 128 + t * 32 + l31, ch)]);
#pragma unroll
        for (int t = 0; t < 2; t++) f.b[t] = *reinterpret_cast<const f32x4 *>(&Bs[wswz(wc * 64 + t * 32 + l31, ch)]);
    };
    // sub-step 0 of the stage in `slot` (F0 holds its fragments on entry, F1 sub-step 1's on exit).  The scheduling fences
    // pin the order written here: the DMA is inline asm, which the scheduler's instruction groups do not see.
    auto sub0 = [&](int slot) {
        wide_mfma<0, 2>(acc, F0);
        __builtin_amdgcn_sched_barrier(0);
        ldfrag(F1, slot, 1);
        __builtin_amdgcn_sched_barrier(0);
        wide_mfma<2, 32>(acc, F0);
        __builtin_amdgcn_sched_barrier(0);
    };
    // sub-step 1 + the next stage's sub-step-0 reads, without / with the 6 pieces of the stage at k0 into dma_slot
    auto sub1 = [&](int next_slot) {
        wide_mfma<0, 2>(acc, F1);
        __builtin_amdgcn_sched_barrier(0);
        ldfrag(F0, next_slot, 0);
        __builtin_amdgcn_sched_barrier(0);
        wide_mfma<2, 32>(acc, F1);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto sub1_dma = [&](int next_slot, int dma_slot, int k0) {
        wide_mfma<0, 2>(acc, F1);
        __builtin_amdgcn_sched_barrier(0);
        ldfrag(F0, next_slot, 0);
        __builtin_amdgcn_sched_barrier(0);
        wide_mfma<2, 8>(acc, F1); // (a piece right behind the reads costs 0.7 % of the headline, LABNOTES R32.1)
        __builtin_amdgcn_sched_barrier(0);
#define LB_W256_PIECE(P)                                \
    piece(P, dma_slot, k0);                             \
    __builtin_amdgcn_sched_barrier(0);                  \
    wide_mfma<8 + 4 * (P), 12 + 4 * (P)>(acc, F1);      \
    __builtin_amdgcn_sched_barrier(0);
        LB_W256_PIECE(0) LB_W256_PIECE(1) LB_W256_PIECE(2) LB_W256_PIECE(3) LB_W256_PIECE(4) LB_W256_PIECE(5)
#undef LB_W256_PIECE
    };
    ldfrag(F0, 0, 0);
    int slot = 0; // ring slot of stage j
    int j = 0;
    for (; j + 3 < nk; j++) {
        const int next = slot == WNST - 1 ? 0 : slot + 1;
        sub0(slot);
        wide_step_barrier<W_NI>(); // stage j+1 is in, stage j+2 may be on its way
        sub1_dma(next, slot, (j + 3) * WBK);
        slot = next;
    }
    if (j + 2 < nk) { // the last step but two: nothing left to request
        const int next = slot == WNST - 1 ? 0 : slot + 1;
        sub0(slot);
        wide_step_barrier<W_NI>();
        sub1(next);
        slot = next;
    }
    { // the last step but one: the last stage is the only one outstanding
        const int next = slot == WNST - 1 ? 0 : slot + 1;
        sub0(slot);
        wide_step_barrier<0>();
        sub1(next);
        slot = next;
    }
    // the last step: no barrier, the ring is not written again
    sub0(slot);
    wide_mfma<0, 32>(acc, F1);
    __builtin_amdgcn_sched_barrier(0); // (the epilogue's keys stay behind the fragments' last use: both do not fit the registers)

    // ---- epilogue: key + admission -------------------------------------------------
    // C layout (32x32): col = lane&31 (query), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).  A lane holds 64 rows per query.
    // Pass 1 (branch-free) builds a 64-bit admission word per query, the side inputs of one 32-row block at a time; then ONE
    // returning atomic per lane and query reserves the slots, and the blocks with admissions are walked again (side inputs
    // read again from LDS, keys computed again: kept next to the 128 accumulators they would not fit the registers).
    uint64_t bits[2] = {0ull, 0ull};
#pragma unroll
    for (int tm = 0; tm < 4; tm++) {
        float aux[4][4];
        uint32_t rid[4][4];
        uint32_t vb = 0; // bit (g*4 + e): row visible (in range and not masked out)
#pragma unroll
        for (int g = 0; g < 4; g++) vb |= tile_rows4(s_aux, s_rowid, s_vis, wr * 128 + tm * 32 + 8 * g + 4 * h, aux[g], rid[g]) << (g * 4);
#pragma unroll
        for (int tn = 0; tn < 2; tn++) {
            uint32_t bb = 0;
#pragma unroll
            for (int g = 0; g < 4; g++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    bb |= admit_exact(cand_key<METRIC>(acc[tm][tn][4 * g + e], aux[g][e]), rid[g][e], tau_key[tn], tau_row[tn]) << (g * 4 + e);
                }
            bits[tn] |= (uint64_t)(bb & vb) << (tm * 16);
        }
        __builtin_amdgcn_sched_barrier(0); // one block's side inputs at a time (hoisted, the four blocks' loads spill)
    }
    // (opaque to the compiler: both admission words exist here -- the second query's test does not sink behind the first
    // query's stores with all its side inputs -- and the second pass reads its side inputs again, behind its branches)
    int lr2 = wr * 128 + 4 * h;
    asm volatile("" : "+v"(lr2), "+v"(bits[0]), "+v"(bits[1]));
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        if (!bits[tn]) continue;
        const int qj = q0 + wc * 64 + tn * 32 + l31; // (a query beyond nq admits nothing: its tau decodes to NaN)
        uint64_t *list = a.cs.lists + (size_t)qj * a.cs.cap;
        uint32_t pos = atomicAdd(&a.cs.cnt[qj], (uint32_t)__builtin_popcountll(bits[tn]));
#pragma unroll
        for (int tm = 0; tm < 4; tm++) {
            const uint32_t bb = (uint32_t)(bits[tn] >> (tm * 16)) & 0xffffu;
            if (!bb) continue;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const uint32_t nib = (bb >> (g * 4)) & 15u;
                if (!nib) continue;
                float aux[4];
                uint32_t rid[4];
                (void)tile_rows4(s_aux, s_rowid, s_vis, lr2 + tm * 32 + 8 * g, aux, rid);
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (nib & (1u << e)) {
                        if (pos < a.cs.cap) list[pos] = pack_entry(cand_key<METRIC>(acc[tm][tn][4 * g + e], aux[e]), rid[e]);
                        pos++;
                    }
            }
        }
    }
}

// f32 [rows][D] -> split-bf16 image of the same byte shape (D % 32 == 0): per row and 16-k group,
// 16 bf16 hi values (x rounded to nearest even) then 16 bf16 lo values (x - hi rounded): one MFMA k-block per 64 B.
__global__ __launch_bounds__(256) void split_bf16_kernel(const float *src, float *dst, int64_t n8)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        bf16x8 hi, lo;
        split_bf16x8(*reinterpret_cast<const f32x4 *>(src + i * 8), *reinterpret_cast<const f32x4 *>(src + i * 8 + 4), hi, lo);
        const int64_t grp = i >> 1; // 16-k group index over the flattened [rows*D/16]
        const int kb = (int)(i & 1);
        char *g = reinterpret_cast<char *>(dst) + grp * 64;
        *reinterpret_cast<bf16x8 *>(g + kb * 16) = hi;
        *reinterpret_cast<bf16x8 *>(g + 32 + kb * 16) = lo;
    }
}

void launch_split_bf16(const float *src, float *dst, int64_t rows, int D, hipStream_t s)
{
    const int64_t n8 = rows * (int64_t)D / 8;
    if (n8 <= 0) return;
    int64_t blocks = (n8 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, n8);
}

// The 256-row body takes a non-boot pass of at least this many of its workgroups (below that the 128-row tile fills the chip
// better: level at 3,900, ahead by 1.3 % at 7,800; sweep in LABNOTES R32.1).
constexpr int kWide256MinTiles = 6144;
#ifdef LB_DIAG
static std::atomic<int> g_wide256_min_tiles{kWide256MinTiles}; // lb_debug_set_wide256_min_tiles
static std::atomic<int> g_last_wide_rows{0};                   // lb_debug_last_wide_rows
#endif

void launch_gemm_filter(int metric, const float *X, const float *norm2, const float *rnorm,
                        int64_t row_begin, int64_t row_end, int D, const float *Q, int nq,
                        const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool boot, hipStream_t s)
{
    if (row_end <= row_begin || nq <= 0) return;
    GemmArgs a;
    a.rowmap = rowmap;
    a.boot = boot ? 1 : 0;
    a.X = X; a.norm2 = norm2; a.rnorm = rnorm;
    a.row_begin = row_begin; a.row_end = row_end; a.D = D;
    a.Q = Q; a.nq = nq; a.mask = mask; a.cs = cs;
    a.n_q_tiles = (nq + BN - 1) / BN;
    const bool aligned = (D % 4 == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0) &&
                         ((reinterpret_cast<uintptr_t>(Q) & 15) == 0);
    const int mode = !aligned ? 0 : (D % BK == 0 ? 2 : 1);
#ifdef LB_DIAG
    const int wide256_min = g_wide256_min_tiles.load(std::memory_order_relaxed);
#else
    const int wide256_min = kWide256MinTiles;
#endif
    const int64_t tiles256 = (row_end - row_begin + WBM - 1) / WBM;
    const bool wide256 = !boot && mode == 2 && tiles256 * a.n_q_tiles >= wide256_min;
#ifdef LB_DIAG
    if (!boot) g_last_wide_rows.store(wide256 ? WBM : BM, std::memory_order_relaxed);
#endif
    a.n_row_tiles = wide256 ? (int)tiles256 : (int)((row_end - row_begin + BM - 1) / BM);
    const int groups = (a.n_row_tiles + 7) / 8;
    dim3 grid((unsigned)(groups * 8 * a.n_q_tiles));
#define LB_GEMM(M, AL) hipLaunchKernelGGL((gemm_filter_kernel<M, AL>), grid, dim3(GEMM_THREADS), 0, s, a)
#define LB_GEMM_M(M)                 \
    do {                             \
        if (wide256) hipLaunchKernelGGL((gemm_filter_wide256_kernel<M>), grid, dim3(GEMM_THREADS), 0, s, a); \
        else if (mode == 2) LB_GEMM(M, 2); \
        else if (mode == 1) LB_GEMM(M, 1); \
        else LB_GEMM(M, 0);           \
    } while (0)
    if (metric == METRIC_L2) LB_GEMM_M(METRIC_L2);
    else if (metric == METRIC_COS) LB_GEMM_M(METRIC_COS);
    else LB_GEMM_M(METRIC_DOT);
#undef LB_GEMM_M
#undef LB_GEMM
}

} // namespace lb

#ifdef LB_DIAG
extern "C" {
int lb_debug_last_wide_rows(void) { return lb::g_last_wide_rows.load(); } // 128 or 256: the tile of the most recent non-boot launch_gemm_filter (0: none yet)
// workgroups from which the 256-row body runs (negative: the compiled-in default); forgets the last launch's tile
void lb_debug_set_wide256_min_tiles(int v)
{
    lb::g_wide256_min_tiles.store(v < 0 ? lb::kWide256MinTiles : v);
    lb::g_last_wide_rows.store(0);
}
}
#endif
