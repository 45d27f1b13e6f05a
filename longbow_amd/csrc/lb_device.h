// lb_device.h -- shared device helpers and kernel-launcher prototypes (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace lb {

// Numeric tunables (thresholds and sizes).  In the product build every tunable IS its compiled-in default (the measured
// winner); only a -DLB_DIAG build (python -m longbow_amd.build --diag -> liblongbow_gpu_diag.so, used by tests/ and tools/)
// reads the LB_* environment variables.
inline int lb_tunable(const char *name, int dflt)
{
#ifdef LB_DIAG
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

// ---------------------------------------------------------------------------
// Candidate entries: (key f32, row u32) packed into one u64 so that unsigned
// integer order == ascending (key, row).  All selection works on these.
// ---------------------------------------------------------------------------
constexpr uint64_t kEntryMax = ~0ull;

__host__ __device__ __forceinline__ uint32_t f32_sortable(float f)
{
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float sortable_f32(uint32_t s)
{
    uint32_t u = (s & 0x80000000u) ? (s & 0x7fffffffu) : ~s;
    return __builtin_bit_cast(float, u);
}
// Canonical order of the reported lists: ascending distance, every NaN after +inf (whatever its sign
// bit), ties by row.  (The reference's heap has no defined behaviour for NaN distances -- a NaN never
// displaces anything, adaptive_index.go:206 -- so this only fixes what it leaves open.)
__host__ __device__ __forceinline__ uint64_t pack_entry(float key, uint32_t row)
{
    key = key + 0.0f; // -0 -> +0
    const uint32_t sk = (key != key) ? 0xffc00000u /* sortable image of the positive quiet NaN */ : f32_sortable(key);
    return ((uint64_t)sk << 32) | row;
}
__host__ __device__ __forceinline__ float entry_key(uint64_t e) { return sortable_f32((uint32_t)(e >> 32)); }
__host__ __device__ __forceinline__ uint32_t entry_row(uint64_t e) { return (uint32_t)e; }
// Threshold in the (key, row) form the MFMA kernels test in the float domain.  "No threshold yet"
// (kEntryMax: e.g. a bootstrap chunk with fewer visible rows than candidates to keep) decodes to
// a NaN key, which would admit nothing -- it must admit every row instead.
__host__ __device__ __forceinline__ float tau_key_of(uint64_t tau)
{
    return tau == ~0ull ? __builtin_huge_valf() : entry_key(tau);
}

inline uint32_t next_pow2_host(uint32_t v)
{
    uint32_t p = 2;
    while (p < v) p <<= 1;
    return p;
}

// Chunk schedule shared by every top-k pipeline (host side).  Chunk 0 is the bootstrap chunk
// (all rows stored, no atomics); every later chunk is sized so that, with the threshold left by
// the previous select (pass rate ~ keep/pos on exchangeable data), about (cap-keep)/4 entries
// are admitted.  safe = chunks that cannot overflow whatever the data order.
// big_boot: use the whole list as bootstrap chunk (scan pipelines: one select level fewer).
inline int64_t chunk_end_host(int step, int64_t pos, int64_t n, int64_t keep, int64_t cap, bool safe,
                              bool big_boot = false)
{
    int64_t end;
    if (step == 0) {
        int64_t boot = 4 * keep > 2048 ? 4 * keep : 2048;
        if (boot > cap || big_boot) boot = cap;
        end = boot;
    } else if (safe) {
        end = pos + (cap - keep);
    } else {
        const int64_t target = (cap - keep) / 4;
        // rows = target * pos / keep, in 128-bit-safe steps
        const double rows = (double)target * (double)pos / (double)(keep > 0 ? keep : 1);
        end = rows > 4e18 ? n : pos + (int64_t)rows;
        if (end <= pos) end = pos + 1;
        if (n - end < end - pos) end = n; // do not leave a tail smaller than this chunk
    }
    return end < n ? end : n;
}

enum : int { METRIC_L2 = 0, METRIC_COS = 1, METRIC_DOT = 2 };
enum : int { ORDER_SEQ = 0, ORDER_UNROLL4 = 1 };

// Per-search candidate state, one slot per query (all in HBM).
struct CandState {
    uint64_t *lists; // [nq][cap] entries; [0,cnt) valid
    uint32_t *cnt;   // [nq] appended so far (may exceed cap -> overflow)
    uint64_t *tau;   // [nq] admission threshold: entry admitted iff e < tau
    uint32_t *flags; // [nq] bit0 = list overflowed, bit1 = containment bound failed, bit2 = sampled threshold too tight
    uint32_t cap;
    // Optional (scan path, sampled pass): 16 admission counters per slot, LB_STRIPE_PAD u32 apart.  Stripe s
    // hands out list positions s, s+16, s+32, ... so the admissions of one query do not serialise on a
    // single hot counter; the following select reads the counters and skips the holes.
    uint32_t *stripes;
};
constexpr int LB_STRIPES = 16;
constexpr int LB_STRIPE_PAD = 32; // u32 words between counters (128 B)

#ifdef __HIPCC__
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- LDS-DMA (global_load_lds_dwordx4: 16 B per lane straight into LDS at M0 + 16 lane) -----------------------------
// Several requests behind ONE M0 write: the instruction offset moves the LDS destination and the global address alike by
// 1 KiB per request (the callers pre-compensate the sources).  An M0 write behind a request has to wait until the
// vector-memory unit has taken that request -- with one M0 value per request every request cost the wave its full acceptance
// time, one M0 write per group lets the requests of a group queue back to back.
// NT: non-temporal (a corpus line that only this workgroup will read).  These carry a "memory" clobber.
template <bool NT>
__device__ __forceinline__ void lds_dma16x4(const void *g0, const void *g1, const void *g2, const void *g3, uint32_t lds_addr)
{
    uint32_t save;
    if (NT)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, off nt\n\t"
                     "global_load_lds_dwordx4 %2, off offset:1024 nt\n\t"
                     "global_load_lds_dwordx4 %3, off offset:2048 nt\n\t"
                     "global_load_lds_dwordx4 %4, off offset:3072 nt\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(save) : "v"(g0), "v"(g1), "v"(g2), "v"(g3), "s"(lds_addr) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, off\n\t"
                     "global_load_lds_dwordx4 %2, off offset:1024\n\t"
                     "global_load_lds_dwordx4 %3, off offset:2048\n\t"
                     "global_load_lds_dwordx4 %4, off offset:3072\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(save) : "v"(g0), "v"(g1), "v"(g2), "v"(g3), "s"(lds_addr) : "memory");
}
__device__ __forceinline__ void lds_dma16x2(const void *g0, const void *g1, uint32_t lds_addr)
{
    uint32_t save;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\t"
                 "global_load_lds_dwordx4 %2, off offset:1024\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(save) : "v"(g0), "v"(g1), "s"(lds_addr) : "memory");
}
// ONE request, WITHOUT a "memory" clobber (requests issued one at a time between the MFMAs of a step: a clobber there changes
// how the compiler schedules those register-heavy loops; the slot being filled is fenced by barriers)
template <bool NT>
__device__ __forceinline__ void lds_dma16_noclobber(const void *g, uint32_t lds_addr)
{
    uint32_t save;
    if (NT)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, off nt\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(save) : "v"(g), "s"(lds_addr));
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, off\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(save) : "v"(g), "s"(lds_addr));
}
// wait until at most N vector-memory requests of this wave are outstanding (LDS-DMA requests are not tracked by the compiler)
template <int N>
__device__ __forceinline__ void wait_vmcnt()
{
    __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
    asm volatile("" ::: "memory");
}

// ---- conversions ------------------------------------------------------------------------------------------------------
// x (8 consecutive f32 of one row) -> hi = bf16(x) (round to nearest even), lo = bf16(x - hi): x = hi + lo + O(2^-18 |x|).
// The corpus's split image (kernels_gemm.hip: split_bf16_kernel) and the in-register splits of the candidate kernels are
// this one function, so that they give the same bits.
__device__ __forceinline__ void split_bf16x8(const f32x4 x0, const f32x4 x1, bf16x8 &hi, bf16x8 &lo)
{
    const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const __bf16 h = (__bf16)x[i];
        hi[i] = h;
        lo[i] = (__bf16)(x[i] - (float)h);
    }
}
__device__ __forceinline__ f16x8 cvt_f16x8(const f32x4 x0, const f32x4 x1)
{
    f16x8 r; // round to nearest even (v_cvt_f16_f32 under the default rounding mode)
    r[0] = (_Float16)x0.x; r[1] = (_Float16)x0.y; r[2] = (_Float16)x0.z; r[3] = (_Float16)x0.w;
    r[4] = (_Float16)x1.x; r[5] = (_Float16)x1.y; r[6] = (_Float16)x1.z; r[7] = (_Float16)x1.w;
    return r;
}

// ---- lane moves on the DPP path (no LDS round trips) ------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v)
{
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    return ((uint64_t)(uint32_t)ohi << 32) | (uint64_t)(uint32_t)olo;
}
// u64 minimum over lanes; shared by the threshold kernels
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t min_dpp_u64(uint64_t v)
{
    const uint64_t o = dpp_u64<CTRL, ROW_MASK>(v);
    return o < v ? o : v;
}
// minimum over each row of 16 lanes, left in every lane of the row
__device__ __forceinline__ uint64_t row16_min_u64(uint64_t v)
{
    v = min_dpp_u64<0xB1, 0xf>(v);  // quad_perm [1,0,3,2]
    v = min_dpp_u64<0x4E, 0xf>(v);  // quad_perm [2,3,0,1]
    v = min_dpp_u64<0x141, 0xf>(v); // row_half_mirror
    v = min_dpp_u64<0x140, 0xf>(v); // row_mirror
    return v;
}
// minimum over the 64 lanes, returned wave-uniform
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
    v = row16_min_u64(v);
    v = min_dpp_u64<0x142, 0xa>(v); // row_bcast15: rows 1,3 <- lane 15 of rows 0,2
    v = min_dpp_u64<0x143, 0xc>(v); // row_bcast31: rows 2,3 <- lane 31
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((uint64_t)hi << 32) | lo;
}

// the same on 32-bit keys (one v_min_u32 with a DPP operand per step)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t min_dpp_u32(uint32_t v)
{
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);
    return o < v ? o : v;
}
__device__ __forceinline__ uint32_t row16_min_u32(uint32_t v)
{
    v = min_dpp_u32<0xB1, 0xf>(v);
    v = min_dpp_u32<0x4E, 0xf>(v);
    v = min_dpp_u32<0x141, 0xf>(v);
    v = min_dpp_u32<0x140, 0xf>(v);
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
    v = row16_min_u32(v);
    v = min_dpp_u32<0x142, 0xa>(v);
    v = min_dpp_u32<0x143, 0xc>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

#endif

// ---------------------------------------------------------------------------
// Launchers (implemented in kernels_*.hip).  All are asynchronous on `s`.
// ---------------------------------------------------------------------------

// per-row ||x||^2 and 1/||x|| (0 if the norm is 0); max ||x||^2 folded into d_maxnorm2[0], the smallest NON-ZERO ||x||^2
// into d_maxnorm2[1] (float bits; initialise to {0, 0x7f800000})
// center (or null): norms of x - center instead (rnorm may then be null)
void launch_row_norms(const float *X, int64_t n, int D, float *norm2, float *rnorm,
                      uint32_t *d_maxnorm2, hipStream_t s, const float *center = nullptr);
// the same over an fp16 index's rows (each element widened to f32 exactly)
void launch_row_norms(const _Float16 *X, int64_t n, int D, float *norm2, float *rnorm, uint32_t *d_maxnorm2, hipStream_t s,
                      const float *center = nullptr);
// n fp16 values (IEEE binary16 bit patterns) -> f32, exactly
void launch_widen_f16(const void *src, float *dst, int64_t n, hipStream_t s);

// ---- the int8 index (kernels_i8.hip): exact values of the reference's int8 registry kernels, candidate entries as the scan's
// per row: the exact sum of x_i^2 over i < 16 floor(D / 16), as int32
void launch_row_norms_i8(const int8_t *X, int64_t n, int D, int32_t *norm2, hipStream_t s);
// n int8 values -> f32, exactly
void launch_widen_i8(const void *src, float *dst, int64_t n, hipStream_t s);
// the scan over int8 rows (launch_scan's contract; Q: int8 queries widened to f32; norm2: launch_row_norms_i8's)
void launch_scan_i8(int metric, const int8_t *X, int64_t row_begin, int64_t row_end, int D, const float *Q, const int *qsel,
                    int nsel, const int32_t *norm2, const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool boot,
                    hipStream_t s, bool striped);
// launch_sample_scores over int8 rows: the sampled entries carry the exact values
void launch_sample_scores_i8(int metric, const int8_t *X, int D, int64_t span, uint32_t count, const uint32_t *rowmap,
                             const uint8_t *mask, const float *Q, const int *qsel, int nsel, CandState cs, hipStream_t s);
// the i8 MFMA pass over npos positions for queries 0 .. nq (int8, Q8): sample = false admits exact entries below tau (row
// view: rowmap / mask); sample = true writes every entry of the npos sampled positions of [0, span) to lists[q][position]
bool mfma_i8_supported(int metric, int D, const void *X, const void *Q8);
void launch_mfma_i8(int metric, const int8_t *X, int64_t npos, int D, const int8_t *Q8, int nq, const int32_t *qn,
                    const int32_t *norm2, const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool sample, int64_t span,
                    hipStream_t s);
// exact |q|^2 of nq int8 queries
void launch_query_norms_i8(const int8_t *Q8, int nq, int D, int32_t *qn, hipStream_t s);
// column means of X[0 .. n) in a fixed order -> center[0 .. Dpad) (zero beyond D); partial: [256][D] scratch
void launch_column_means(const float *X, int64_t n, int D, float *partial, float *center, int Dpad, hipStream_t s);
void launch_column_means(const _Float16 *X, int64_t n, int D, float *partial, float *center, int Dpad, hipStream_t s);

// candidate generation: f32 MFMA inner products of queries [nq][D] x rows [row_begin,row_end)
// -> metric key -> admit (key,row) < tau[q] into the query's list.
// boot: every row is stored at list[row - row_begin] (no admission test, no atomics).
void launch_gemm_filter(int metric, const float *X, const float *norm2, const float *rnorm,
                        int64_t row_begin, int64_t row_end, int D, const float *Q, int nq,
                        const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool boot, hipStream_t s);
// small/mid-size batches (5..384 queries): 256-row x 32-query tiles, HBM-bound; needs D % 32 == 0, 16-B aligned X/Q
void launch_gemm_filter_narrow(int metric, const float *X, const float *norm2, const float *rnorm,
                               int64_t row_begin, int64_t row_end, int D, const float *Q, int nq,
                               const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool boot,
                               hipStream_t s, bool tile64 = false); // tile64: 128 rows x 64 queries per workgroup
// Sampled threshold fused into the candidate pass (kernels_gemm_narrow.hip, FUSED): the first `n_blocks` workgroups of
// the launch score `count` sampled rows (corpus rows smap[0..count)), then workgroup j < nq turns query j's sample keys
// into tau[j] (the m-th smallest), zeroes cnt[j] / flags[j], writes the exact ||q_j||^2 (cosine) and publishes
// ready[j] = epoch; the corpus tiles of the same launch pick the thresholds up in front of their epilogues.
// ticket: a counter that only grows (every sample workgroup adds 1); ticket_base = its value before this launch.
struct FusedSample {
    const uint32_t *smap = nullptr;
    uint32_t count = 0;
    int m = 0;
    uint32_t n_blocks = 0;
    uint32_t *ticket = nullptr;
    uint32_t ticket_base = 0;
    uint32_t *ready = nullptr;
    uint32_t epoch = 0;
    float *qna = nullptr; // or null (not cosine)
    int order = 0;
    uint32_t *fail_host = nullptr; // pinned: set to `epoch` when a wait gave up (the host then redoes the batch exactly)
};
void launch_gemm_filter_narrow_fused(int metric, const float *X, const float *norm2, const float *rnorm, int64_t row_begin,
                                     int64_t row_end, int D, const float *Q, int nq, const uint8_t *mask,
                                     const uint32_t *rowmap, CandState cs, hipStream_t s, bool tile64, FusedSample fs);
uint32_t fused_sample_blocks(uint32_t count, int nq, bool tile64); // sample workgroups such a launch starts with
// f32 [rows][D] -> split-bf16 image (same byte shape; D % 32 == 0) consumed by the split GEMM
void launch_split_bf16(const float *src, float *dst, int64_t rows, int D, hipStream_t s);
// split-bf16 contraction on 256 x 256 tiles with whole 128-B lines per row and K-step (kernels_gemm_tall2.hip); Qs = split image
// of the batch (launch_split_bf16); asplit 1: X is the split image of the corpus, 2: X is the f32 corpus (split in registers)
void launch_gemm_filter_tall2(int metric, const float *X, const float *norm2, const float *rnorm, int64_t row_begin,
                              int64_t row_end, int D, const float *Qs, int nq, const uint8_t *mask, const uint32_t *rowmap,
                              CandState cs, bool boot, int asplit, hipStream_t s);

// ONE fp16 product per (row, query, k) on 256 x 256 tiles (kernels_gemm_tall16.hip): Qh / qinv from launch_query_prep
// (fp16 image of the batch, each query scaled by a power of two to a norm in [1, 2); qinv = 1 / scale); X = f32 corpus
//
// The one-tile persistent kernel over the image (<= 128 queries) can turn the sample the launch before it left in
// lists[q][0 .. count) into the thresholds ITSELF (its first nq workgroups do, on shorter row ranges; everybody picks the
// thresholds up in front of its first epilogue): no threshold launch, no gap behind it.  The launch before must leave
// tau[q] = 0 ("not out yet": launch_query_prep / SamplePrep, tau_zero); a bounded wait that gives up stores `tag` to the
// pinned fail_host and admits nothing (the host redoes the batch).  Q / qna / order: the duty workgroups also compute the
// exact ||q||^2 (cosine; qna null otherwise).
struct Tall16Tin {
    uint32_t count;
    int m;
    uint32_t tag;
    uint32_t *fail_host;
    const float *Q;
    float *qna;
    int order;
#ifdef LB_DIAG
    int withhold; // the duty workgroups keep their thresholds: every wave's bounded wait gives up (lb_debug_tin_withhold_next)
#endif
};
bool tall16_tin_ok(int D, int nq, int64_t n_pos, bool img, bool mapped, bool masked, bool with_norm, uint32_t count, int m);
// that image and those scales, plus the exact ||q||^2 in `order` (qna, or null) and the reset of the queries' candidate state:
// one launch for what a search over this route needs from its batch (kernels_scan.hip)
void launch_query_prep(const float *Q, int nq, int D, void *Qh, float *qinv, float *qna, int order, CandState cs, hipStream_t s,
                       const float *center = nullptr, // center: the image of q - center (L2 over the centred corpus image)
                       float *qnrm = nullptr,         // [nq] upper bounds of |q| (the dot product's lower-bound key)
                       bool tau_zero = false,         // thresholds left at 0 = "not out yet" (a TAUIN candidate launch follows)
                       float *qrho = nullptr,         // [nq] |q - fp16 image of q| / |q|, padded: the query's share of the keys' error bound
                       float rho_gain = 0.f);         // qnrm[q] *= 1 + rho_gain * qrho[q] (dot product: folds that share into G)
// Xh (or null): the corpus's K-blocked fp16 image [Dp / 32][xh_cap][32] from launch_corpus_to_f16, in step with X; used by
// unfiltered searches (half the bytes to stage, a four-stage ring)
void launch_gemm_filter_tall16(int metric, const float *X, const float *norm2, const float *rnorm, int64_t row_begin,
                               int64_t row_end, int D, const void *Qh, const float *qinv, int nq, const uint8_t *mask,
                               const uint32_t *rowmap, CandState cs, bool boot, hipStream_t s, const void *Xh = nullptr,
                               int64_t xh_cap = 0,
                               uint32_t gstride = 0,  // boot launches of the persistent forms: positions = granules of 16 rows,
                                                      // gstride rows apart (an evenly spaced sample read in whole KiB)
                               const float *qnrm = nullptr, float gsum = 0.f, // dot product on the persistent forms: upper bounds
                                                      // of |q| (launch_query_prep) and gamma_a + gamma_o -- the lower-bound key
                               const struct Tall16Tin *tin = nullptr); // thresholds inside the launch (tall16_tin_ok)
void launch_corpus_to_f16(const float *X, int64_t row_begin, int64_t row_end, int D, void *Xh, int64_t cap, hipStream_t s,
                          const float *center = nullptr);
// the same from an fp16 index's rows: a relayout (exact), or fp16(x - center) with the subtraction in f32
void launch_corpus_to_f16(const _Float16 *X, int64_t row_begin, int64_t row_end, int D, void *Xh, int64_t cap, hipStream_t s,
                          const float *center = nullptr); // center (or null; [>= D + 8]): the image holds fp16(x - center)
// *stat = max(*stat, max over the rows of |x - fp16(x)|^2 / |x|^2) as float bits (x - center for the centred image): the
// measured loss of the image, from which the candidate keys' error bound is taken (index_search.hip: gamma)
void launch_f16_residual(const float *X, int64_t row_begin, int64_t row_end, int D, const float *center, uint32_t *stat, hipStream_t s);
void launch_f16_residual(const _Float16 *X, int64_t row_begin, int64_t row_end, int D, const float *center, uint32_t *stat, hipStream_t s);
int corpus_f16_plane_dims(); // dimensions per plane of that image (its rows are zero-padded to a multiple of it)
// under a row list (mapped) the persistent kernels gather out of the image and leave POSITIONS of the list in the candidate
// entries (the finish launch maps them back: posmap); true when a launch with these parameters does so
bool tall16_entries_are_positions(int D, int nq, bool img, bool mapped, bool masked);
bool tall16_runs_persistent(int D, int nq, bool img, bool mapped, bool masked); // the persistent kernels serve such a launch

// per query: sort the list, keep the best kc, tau = kc-th entry (or max), flag overflow.
// qsel (nullable): only these query slots.  boot_rows > 0: the list was filled by a bootstrap
// launch (one entry per row at index row - row_begin, no atomics; masked rows hold kEntryMax).
// need_at_least: flag bit 2 when fewer entries than this were admitted (sampled threshold too tight).
// emit: the search's last select also writes the k results per slot (what launch_emit_lists would do)
struct EmitArgs {
    int k;
    const int64_t *ids;
    float *out_dist;
    int64_t *out_labels;
    uint32_t *flags_host;
};
void launch_select(CandState cs, const int *qsel, int nsel, int kc, uint32_t boot_rows, hipStream_t s,
                   uint32_t need_at_least = 0, const EmitArgs *emit = nullptr,
                   bool striped = false,
                   bool unsorted = false); // unsorted: the kept entries need not be ordered, only the worst one sits last
// approximate distances of `count` evenly spaced positions of [0, span) for up to 8 query slots, written
// as entries to lists[q][0..count) (also clears the slots' flags); cosine: `nsel` extra workgroups compute
// the slots' exact ||q||^2 into qna in the requested order.  norm2/rnorm given ("keys" mode, up to 64 slots):
// the entries carry the MFMA pipeline's candidate keys instead of distances
// prep (or null): the launch also does launch_query_prep's work for its queries (image, scales, |q| bounds; not the exact
// norms, not the state reset -- the threshold launch behind it sets the state): one launch and one gap less in front of a
// small search's candidate pass
struct SamplePrep {
    void *Qh;
    float *qinv, *qnrm;
    const float *center;
    bool tau_zero; // leave tau = 0 ("not out yet": a TAUIN candidate launch follows)
    float *qrho;   // as launch_query_prep
    float rho_gain;
};
void launch_sample_scores(int metric, int order, const float *X, int D, int64_t span, uint32_t count,
                          const uint32_t *rowmap, const uint8_t *mask, const float *Q, const int *qsel, int nsel,
                          CandState cs, float *qna, hipStream_t s, const float *norm2 = nullptr,
                          const float *rnorm = nullptr,
                          const float *center = nullptr,  // keys mode, L2: keys about this centre (norm2 = the centred norms)
                          const SamplePrep *prep = nullptr);
// the same over an fp16 index's rows (each element widened to f32 exactly)
void launch_sample_scores(int metric, int order, const _Float16 *X, int D, int64_t span, uint32_t count,
                          const uint32_t *rowmap, const uint8_t *mask, const float *Q, const int *qsel, int nsel,
                          CandState cs, float *qna, hipStream_t s, const float *norm2 = nullptr, const float *rnorm = nullptr,
                          const float *center = nullptr, const SamplePrep *prep = nullptr);
// tau[q] = m-th smallest of lists[q][0..count) with the row bits saturated, cnt[q] = 0
bool sample_tau_supported(uint32_t count, int m);
// zero_stripes: also reset the slots' striped admission counters (at most 8 slots: the scan path)
// qna != null: `nsel` extra workgroups compute the slots' exact ||q||^2 (order) alongside
void launch_sample_tau(CandState cs, const int *qsel, int nsel, uint32_t count, int m, bool zero_stripes, hipStream_t s,
                       const float *Q = nullptr, int D = 0, float *qna = nullptr, int order = 0);
// smap[i] = row behind the i-th of `count` evenly spaced positions of [0, span) (through rowmap if given)
void launch_sample_map(const uint32_t *rowmap, int64_t span, uint32_t count, uint32_t *smap, hipStream_t s);

// The last launch of a batched search (kernels_finish.hip): members of each query's candidate list within the key-space cut
// a_k + (1 + beta) E are re-ranked in the exact order, proven (or flagged: bit 1) and written.  posmap (or null): the lists
// carry positions of this row list.  done / xcnt: [nq] words that are zero between launches; xscratch: finish_scratch_bytes
// for the split form (up to nq_split_max queries); smax: members a query may have (power of two, >= 1024).
size_t finish_scratch_bytes(int nq_split_max, uint32_t smax);
void launch_finish(int metric, int order, const float *X, int D, const float *Q, int nq, const float *qna, CandState cs, int k,
                   const uint32_t *d_maxnorm2, float gamma, float beta, const int64_t *ids, const uint32_t *posmap, float *out_dist,
                   int64_t *out_labels, hipStream_t s, uint32_t *flags_host, uint32_t *done, uint32_t *xcnt, void *xscratch,
                   int nq_split_max, uint32_t smax,
                   const float *center = nullptr, // L2 keys taken about this centre: d_maxnorm2 = the centred maximum norm
                   const float *lb_norm2 = nullptr, const float *lb_qnrm = nullptr, float lb_gsum = 0.f, // dot: lower-bound keys
                   const float *qrho = nullptr, float qrho_k = 0.f);
// the same over an fp16 index's rows (one lane per member, straight from the row)
void launch_finish(int metric, int order, const _Float16 *X, int D, const float *Q, int nq, const float *qna, CandState cs, int k,
                   const uint32_t *d_maxnorm2, float gamma, float beta, const int64_t *ids, const uint32_t *posmap, float *out_dist,
                   int64_t *out_labels, hipStream_t s, uint32_t *flags_host, uint32_t *done, uint32_t *xcnt, void *xscratch,
                   int nq_split_max, uint32_t smax,
                   const float *center = nullptr,
                   const float *lb_norm2 = nullptr, const float *lb_qnrm = nullptr, float lb_gsum = 0.f,
                   const float *qrho = nullptr, float qrho_k = 0.f); // gamma(q) = gamma + qrho_k * qrho[q] (launch_query_prep)

// ||q||^2 per selected query slot in the requested accumulation order (cosine).
void launch_query_norms(int order, const float *Q, const int *qsel, int nsel, int D, float *qna,
                        hipStream_t s);

// exact-order scan (nsel <= 8): distances of every row in [row_begin,row_end) for query slots
// qsel[0..nsel) (indices into Q, or identity when qsel==nullptr), admitted against tau.
// If all_out != nullptr writes every distance to all_out[slot*ld + row] instead (simd batch API).
void launch_scan(int metric, int order, bool raw_dot, const float *X, int64_t row_begin,
                 int64_t row_end, int D, const float *Q, const int *qsel, int nsel,
                 const float *qna, const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool boot,
                 float *all_out, int64_t ld, hipStream_t s, bool striped = false);
// the same over an fp16 index's rows: each element is widened to f32 (exact) and the reference's f32 arithmetic runs on it
void launch_scan(int metric, int order, bool raw_dot, const _Float16 *X, int64_t row_begin,
                 int64_t row_end, int D, const float *Q, const int *qsel, int nsel,
                 const float *qna, const uint8_t *mask, const uint32_t *rowmap, CandState cs, bool boot,
                 float *all_out, int64_t ld, hipStream_t s, bool striped = false);

// after the last select of the scan path: lists already hold exact distances.
void launch_emit_lists(CandState cs, const int *qsel, int nsel, int k, const int64_t *ids,
                       float *out_dist, int64_t *out_labels, uint32_t *flags_host, hipStream_t s);

void launch_init_cand(CandState cs, const int *qsel, int nsel, hipStream_t s);
// dist[0..n) = FLT_MAX, lab[0..n) = -1 (simd_api.hip)
void launch_fill_empty(float *dist, int64_t *lab, int64_t n, hipStream_t s);

// shard s's [nq][k] blocks start at dist_in + s*dist_stride and lab_in + s*lab_stride (elements)
void launch_merge_topk(int nshards, int64_t nq, int k, const float *dist_in, const int64_t *lab_in,
                       int64_t dist_stride, int64_t lab_stride, float *dist_out, int64_t *lab_out, hipStream_t s);

void launch_fill_uniform(float *dst, int64_t n, uint64_t seed, int64_t offset, hipStream_t s);
void launch_fill_codes(uint8_t *dst, int64_t n, uint64_t seed, int64_t offset, hipStream_t s);
void launch_fill_uniform_rows(float *dst, const int64_t *ids, int64_t nrows, int dim, uint64_t seed, hipStream_t s);

// PQ
// minrng (nullable): [nq][M][4] = {min, max - min, 1.0 if the subtable holds a NaN / negative / infinite entry, 0}
void launch_build_adc_table(const float *codebooks, int M, int K, int sub, const float *Q, int nq,
                            float *tables, hipStream_t s, float *minrng = nullptr,
                            uint32_t *zero_a = nullptr, uint32_t *zero_b = nullptr); // zero_*: [nq] words cleared on the way
// one query per launch: `table` is that query's [M*256] table; entries go to cs slot `slot`,
// or (all_out != nullptr) every distance is written to all_out[row - out_base].
// skip_if_ok (nullable): {s_tau, ok} of the byte-table prefilter; the launch returns at once when ok != 0
// (the prefilter + exact-candidates kernels did the work)
void launch_adc_scan(const float *table, int M, const uint8_t *codes, int64_t row_begin, int64_t row_end,
                     int slot, const uint8_t *mask, CandState cs, bool boot, float *all_out,
                     int64_t out_base, hipStream_t s, const int *skip_if_ok = nullptr);

// sampled threshold for the ADC scan: exact ADC entries of `count` evenly spaced rows -> out[count];
// launch_sample_topm reduces them to groups*m entries at lists[slot] (returns groups, 0 = does not fit)
void launch_adc_sample(const float *table, int M, const uint8_t *codes, int64_t n, uint32_t count, uint64_t *out,
                       hipStream_t s);
uint32_t launch_sample_topm(const uint64_t *in, uint32_t count_total, int m, CandState cs, int slot, hipStream_t s);

// PQ codec + two-stage ADC search (kernels_pq2.hip)
void launch_pq_encode(const float *codebooks, int M, int K, int sub, const float *X, int64_t n, uint8_t *codes,
                      hipStream_t s);
void launch_pq_decode(const float *codebooks, int M, int K, int sub, const uint8_t *codes, int64_t n, float *out,
                      hipStream_t s);
// PQ training (kernels_pq_train.hip): Lloyd k-means per subspace, all M subspaces in every launch.  The state as the kernels
// take it (by value); n < 2^31, K <= 256.
constexpr int KM_CHUNK = 4096; // rows per unit of the stable ordering (a multiple of the E-step's 256 rows)
struct KmState {
    const float *X;       // [n][D] rows, resident for the whole call
    int64_t n, nchunks;   // nchunks = ceil(n / KM_CHUNK)
    int D, M, K, sub;
    float *cent;          // [M][K][sub]
    int32_t *assign;      // [M][n], -1 before the first iteration
    uint32_t *order;      // [M][n] rows sorted by (assignment, row)
    uint32_t *chunk_hist; // [M][nchunks][K] zero between iterations
    uint32_t *count, *start; // [M][K]
    uint32_t *changed;    // [M]
    uint32_t *done;       // [M] 1 = the subspace has stopped: every launch skips it
    int32_t *iters;       // [M] iterations run
    uint32_t *bad;        // [1] a row had no centroid below FLT_MAX: the call fails
};
uint64_t km_draw(uint64_t seed, uint64_t m, uint64_t t);
void launch_km_init(const KmState &st, const int64_t *d_init_rows, hipStream_t s);
void launch_km_estep(const KmState &st, hipStream_t s);
void launch_km_order(const KmState &st, hipStream_t s);
void launch_km_mstep(const KmState &st, uint64_t seed, int it, hipStream_t s);
// h_state (pinned): {subspaces that go on, bad}
void launch_km_finish(const KmState &st, int it, uint32_t thr, uint32_t *h_state, hipStream_t s);

// byte table + integer admission bound of one query: params = {s_tau, ok}; minrng from launch_build_adc_table
void launch_adc_quantise(const float *table, const float *minrng, int M, const uint64_t *tau, uint8_t *qtab, int *params,
                         hipStream_t s);
// rows whose lower bound can still pass the slot's threshold -> cand[0..*cand_cnt) (false: M too large for LDS)
bool launch_adc_prefilter(const uint8_t *qtab, const int *params, int M, const uint8_t *codes, int64_t n,
                          uint32_t *cand, uint32_t cand_cap, uint32_t *cand_cnt, hipStream_t s);
// two queries in ONE pass over the codes (false: no such form for this M -- run two single passes)
bool launch_adc_prefilter2(const uint8_t *qtab, const int *params, uint32_t *cand, uint32_t *cand_cnt, const uint8_t *qtab2,
                           const int *params2, uint32_t *cand2, uint32_t *cand_cnt2, int M, const uint8_t *codes, int64_t n,
                           uint32_t cand_cap, hipStream_t s);
// four queries in ONE pass (interleaved byte tables, one dword gather per code byte; false: no such form for this M)
bool launch_adc_prefilter4(const uint8_t *const qtab[4], const int *const params[4], uint32_t *const cand[4], uint32_t *const cand_cnt[4],
                           int M, const uint8_t *codes, int64_t n, uint32_t cand_cap, hipStream_t s);
void launch_adc_exact_candidates(const float *table, int M, const uint8_t *codes, const uint32_t *cand,
                                 const uint32_t *cand_cnt, uint32_t cand_cap, const int *params, int slot, CandState cs,
                                 hipStream_t s);
void launch_adc_rerank(const float *table, int M, const uint8_t *codes, int64_t n, const int64_t *rows, int64_t nrows,
                       float *out_dist, float *out_score, hipStream_t s);

// The ADC search under a row filter (kernels_pq_list.hip): the forms of the sample, the exact scan and the prefilter that walk
// POSITIONS of the ascending list of visible rows, rowmap[0, n_vis), and gather each position's code row.  The arithmetic is
// that of the kernels above and the entries / candidates carry corpus rows, so launch_select, launch_adc_exact_candidates and
// the emit follow unchanged.  A zero-length list launches nothing.
constexpr int ADC_LIST_WAVES = 16; // waves per workgroup: a workgroup walks runs of ADC_LIST_WAVES * 64 positions
// exact ADC entries of `count` evenly spaced positions of the list -> out[count] (as launch_adc_sample)
void launch_adc_list_sample(const float *table, int M, const uint8_t *codes, const uint32_t *rowmap, int64_t n_vis,
                            uint32_t count, uint64_t *out, hipStream_t s);
// positions [pos_begin, pos_end) into cs slot `slot`: boot = every position's entry at lists[slot][pos - pos_begin],
// otherwise the entries below the slot's threshold are appended (as launch_adc_scan)
void launch_adc_list_scan(const float *table, int M, const uint8_t *codes, const uint32_t *rowmap, int64_t pos_begin,
                          int64_t pos_end, int slot, CandState cs, bool boot, hipStream_t s);
// as launch_adc_prefilter / launch_adc_prefilter2 over the list (false: no such form, as there)
bool launch_adc_list_prefilter(const uint8_t *qtab, const int *params, int M, const uint8_t *codes, const uint32_t *rowmap,
                               int64_t n_vis, uint32_t *cand, uint32_t cand_cap, uint32_t *cand_cnt, hipStream_t s);
bool launch_adc_list_prefilter2(const uint8_t *qtab, const int *params, uint32_t *cand, uint32_t *cand_cnt, const uint8_t *qtab2,
                                const int *params2, uint32_t *cand2, uint32_t *cand_cnt2, int M, const uint8_t *codes,
                                const uint32_t *rowmap, int64_t n_vis, uint32_t cand_cap, hipStream_t s);

// The tail of a k-NN by counting (kernels_countsel.hip; the method is stated in lb_countsel.h): what the selections of
// kernels_bq.hip and kernels_sq8.hip share once a per-query threshold is known.  Workgroup b of nblk owns the rows of tiles
// [b * tpb, (b + 1) * tpb), 256 rows a tile.  Under a row filter the rows of a search are the positions of the ascending list of
// visible rows: positions order as rows do, so the selection runs over them unchanged and only the finish maps them back.
struct CountSel {
    int64_t n;         // rows the search walks: positions [0, n)
    int k, nq;
    int nblk, tpb;     // countsel_plan(n, max_blocks): workgroups and tiles per workgroup
    uint32_t *thr;     // [nq][2]: threshold t, rows at t that are still needed (0x7fffffff, 0: fewer than k rows, all are below)
    uint32_t *cnt;     // [nq][nblk][2]: rows below t, rows at t; after the scan their exclusive prefixes
    uint32_t *tot;     // [nq]: rows below t
    uint64_t *keys;    // [nq][k]: distance << 32 | position, unordered
};
void countsel_plan(int64_t n, int max_blocks, int *nblk, int *tpb);
void launch_countsel_scan(const CountSel &a, hipStream_t s);
// n == 0 allowed: all padding.  posmap (nullable): the list of visible rows the search walked; the label of position i is
// posmap[i], else i.  (An argument of the one launch that needs it and not a field of CountSel: the argument blocks of every
// other kernel of the two selections, and with them their code, stay what they were.)
void launch_countsel_finish(const CountSel &a, float *dist, int64_t *labels, hipStream_t s, const uint32_t *posmap = nullptr);

// binary-quantised codes (kernels_bq.hip): W = (dims + 63) / 64 u64 words per row, bit i % 64 of word i / 64 is dimension i
void launch_bq_encode(const float *X, int64_t n, int dims, uint64_t *codes, hipStream_t s);
void launch_bq_decode(const uint64_t *codes, int64_t n, int dims, float *out, hipStream_t s);
// out[i] = Hamming distance of stored row row0 + i to qcode, over whole words
void launch_bq_batch(const uint64_t *codes, int W, const uint64_t *qcode, int64_t row0, int64_t n, int32_t *out, hipStream_t s);
// gathered rows: dist = float32(distance), score = 1 - dist / dims (nullable); rows outside [0, ntotal): FLT_MAX / 0
void launch_bq_rerank(const uint64_t *codes, int W, int dims, int64_t ntotal, const uint64_t *qcode, const int64_t *rows, int64_t n,
                      float *dist, float *score, hipStream_t s);
// exact k-NN by counting (lb_countsel.h states the method): the state of one batch of queries as the kernels take it (by
// value); n in 1..2^31-1, k <= 2048.  hist -> thresh -> count -> scan -> emit -> finish, each a launch; hist must be zero
// before the first.
constexpr int BQ_MAX_BLOCKS = 2048; // workgroups that share the rows (each a contiguous range of whole 256-row tiles)
struct BqSearch : CountSel {
    const uint64_t *codes; // [n][W]; under a list [ntotal][W]
    int W;
    const uint64_t *Q;     // [nq][W]
    uint32_t *hist;        // [nq][64*W + 1]
    const uint32_t *rowmap; // nullable: position i is row rowmap[i] (ascending, n of them); last, so that the unmapped kernels'
                            // arguments lie where they did
};
void launch_bq_hist(const BqSearch &a, hipStream_t s);
void launch_bq_thresh(const BqSearch &a, hipStream_t s);
void launch_bq_count(const BqSearch &a, hipStream_t s);
void launch_bq_emit(const BqSearch &a, hipStream_t s);

// scalar-quantised codes (kernels_sq8.hip): one uint8 per dimension, rows stored at `stride` = dims rounded up to 16 bytes with
// zero pad bytes (which add nothing to any sum).  `cstride` arguments are the row stride of a caller's codes (dims when packed).
constexpr int SQ8_MAX_BLOCKS = 1024; // workgroups that share the rows of a search (each a contiguous run of whole 256-row tiles)
constexpr int SQ8_RADIX_BINS = 2048;
inline int sq8_stride(int dims) { return (dims + 15) & ~15; }
// state[2][dims] = {min, max}: seeded from row 0 of X (sq8_bounds_seed), then folded with n rows at a time (sq8_bounds_fold;
// part: scratch of 2 * sq8_bounds_parts(n) * dims floats), in fixed order: reproducible run to run
int sq8_bounds_parts(int64_t n);
void launch_sq8_bounds_seed(const float *X, int dims, float *state, hipStream_t s);
void launch_sq8_bounds_fold(const float *X, int64_t n, int dims, float *part, float *state, hipStream_t s);
// EncodeInto: X f32[n][dims] -> codes u8[n][stride], pad bytes zero
void launch_sq8_encode(const float *X, int64_t n, int dims, const float *mn, const float *mx, const float *scale, uint8_t *codes,
                       hipStream_t s);
// DecodeInto: codes u8[n][cstride] -> out f32[n][dims]
void launch_sq8_decode(const uint8_t *codes, int64_t n, int dims, int cstride, const float *mn, const float *inv, float *out,
                       hipStream_t s);
// dst u8[n][dstride] = the first `width` bytes of each row of src u8[n][sstride], zero beyond them
void launch_sq8_restride(const uint8_t *src, int sstride, uint8_t *dst, int dstride, int width, int64_t n, hipStream_t s);
// norms[r] = sum of squares of the stride bytes of row r
void launch_sq8_norms(const uint8_t *codes, int64_t n, int stride, int32_t *norms, hipStream_t s);
// The distance pass: out[q][i] = S(row row0 + i, query q) for i in [0, n), q in [0, nq); Q u8[nq][stride], qn their norms.
// Under a list (launch_sq8_dist's rowmap: n positions, row0 = 0) position i stands for row rowmap[i].
struct Sq8Dist {
    const uint8_t *codes;  // [ntotal][stride]
    const int32_t *norms;  // [ntotal]
    int stride;
    int64_t row0, n;
    const uint8_t *Q;      // [nq][stride]
    const int32_t *qn;     // [nq]
    int nq;
    int32_t *out;          // [nq][n]
};
// rowmap (nullable): the ascending list of rows to walk.  An argument of its own and not a field of Sq8Dist: behind the struct
// and tpb in the kernel's argument block it leaves the unmapped kernel's arguments, and its code, as they were
void launch_sq8_dist(const Sq8Dist &a, hipStream_t s, const uint32_t *rowmap = nullptr);
// gathered rows, one query u8[dims]: s = S as int32, euclid (nullable) = SQ8EuclideanDistance; rows outside [0, ntotal):
// INT32_MAX / FLT_MAX
void launch_sq8_rerank(const uint8_t *codes, int stride, int dims, int64_t ntotal, const uint8_t *qcode, const int64_t *rows, int64_t n,
                       const float *mn, const float *inv, int32_t *out_s, float *out_euclid, hipStream_t s);
// exact k-NN by counting (lb_countsel.h) over the distances S[nq][n] of one batch of queries (n in 1..2^31-1, k <= 2048):
// (hist, digit) x 3 -> count -> scan -> emit -> finish; hist must be zero before the first.  While the digits are selected
// thr holds the digits found so far and the rank still wanted among them.
struct Sq8Select : CountSel {
    const int32_t *S;  // [nq][n]
    uint32_t *hist;    // [nq][SQ8_RADIX_BINS]
};
void launch_sq8_hist(const Sq8Select &a, int pass, hipStream_t s);
void launch_sq8_digit(const Sq8Select &a, int pass, hipStream_t s);
void launch_sq8_count(const Sq8Select &a, hipStream_t s);
void launch_sq8_emit(const Sq8Select &a, hipStream_t s);

// predicate masks (kernels_filter.hip): op = simd.CompareOp value; validity = Arrow LSB bitmap or null
void launch_match_int64(const int64_t *src, int64_t n, int64_t val, int op, const uint8_t *validity,
                        int64_t valid_offset, uint8_t *dst, int combine, hipStream_t s);
void launch_match_float32(const float *src, int64_t n, float val, int op, const uint8_t *validity,
                          int64_t valid_offset, uint8_t *dst, int combine, hipStream_t s);
void launch_and_bytes(uint8_t *dst, const uint8_t *src, int64_t n, hipStream_t s);
// ordered compaction of a byte mask into the ascending list of visible rows; scratch holds
// compact_scratch_words(n) u32 and ends with the visible-row count at [words-1]
int64_t compact_scratch_words(int64_t n);
void launch_compact_mask(const uint8_t *mask, int64_t n, uint32_t *rowmap, uint32_t *scratch, hipStream_t s);
// its middle step alone: counts[0, nb) -> their exclusive prefix in place, counts[nb] = the total (one workgroup)
void launch_compact_offsets(uint32_t *counts, int64_t nb, hipStream_t s);
// the view of a search call that brings its own row bitmap (kernels_index_call.hip).  d_bits: [ceil(n / 8)] bytes at any address,
// bit r & 7 of byte r >> 3 is row r; hmask: the index's effective mask or null; cmask: the call's mask, 1 where the bit is set and
// hmask (if any) is non-zero, written in whole blocks of INDEX_CALL_BLOCK_ROWS bytes (0 behind row n - 1); scratch:
// compact_scratch_words(n) words.  _bits leaves a count per block in scratch; launch_compact_offsets(scratch, blocks) turns them
// into offsets with the total at scratch[blocks]; _scatter then writes the ascending row list (total entries).
constexpr int INDEX_CALL_BLOCK_ROWS = 2048;
inline int64_t index_call_blocks(int64_t n) { return (n + INDEX_CALL_BLOCK_ROWS - 1) / INDEX_CALL_BLOCK_ROWS; }
void launch_index_call_bits(const uint8_t *d_bits, const uint8_t *hmask, int64_t n, uint8_t *cmask, uint32_t *scratch, hipStream_t s);
void launch_index_call_scatter(const uint8_t *cmask, int64_t n, const uint32_t *scratch, uint32_t *rowmap, hipStream_t s);
// removal and compaction of the flat index (kernels_remove.hip).  live: a byte per row, non-zero = live, held in whole words;
// mask: the index's effective mask.  Both lose the bytes of the rows a call removes; *removed (zero before the launch) gains the
// number of rows that were live before it, each counted once however often it is named.
// rows[cnt]: positions; anything outside [0, ntotal) is skipped
void launch_remove_rows(const int64_t *rows, int64_t cnt, int64_t ntotal, uint8_t *live, uint8_t *mask, uint32_t *removed, hipStream_t s);
// set[nset]: ids, ascending and distinct; every live row r with ids[r] in the set goes
void launch_remove_ids(const int64_t *ids, int64_t ntotal, const int64_t *set, int64_t nset, uint8_t *live, uint8_t *mask,
                       uint32_t *removed, hipStream_t s);
// *out (0xffffffff before the launch) = the first row whose live byte is zero
void launch_first_dead(const uint8_t *live, int64_t ntotal, uint32_t *out, hipStream_t s);
// dst row j = src row map[j] for j < cnt, rows of row_bytes bytes; dst and src must not overlap
void launch_gather_rows(const void *src, const uint32_t *map, int64_t cnt, size_t row_bytes, void *dst, int device, hipStream_t s);
// reciprocal-rank fusion of two ranked id lists per query (kernels_filter.hip)
void launch_rrf(int64_t nq, int kd, const int64_t *dense, int ks, const int64_t *sparse, int k, int limit,
                int64_t *out_ids, float *out_scores, hipStream_t s);

} // namespace lb
