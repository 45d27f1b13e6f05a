// lb_u8_exact.h -- the uint8 arithmetic of one (row, query) pair, for kernels_u8.hip (the flat uint8 index) and
// kernels_ivf_u8.hip (the list scan of a uint8 IVF-Flat handle).  It is the
// reference's only DataTypeUint8 registry kernel, euclideanUint8Unrolled4x (internal/simd/simd_baseline.go:198-220, reached
// through internal/simd/dispatch.go:250):
//   four f32 chains over the residues i mod 4 of i < 4 floor(D / 4), the tail elements into chain 0; each term is
//   d = float32(a_i) - float32(b_i), then d * d (both exact: |d| <= 255), added to its chain in f32, no FMA; the chains are
//   added as ((s0 + s1) + s2) + s3 in f32; the value is float32(sqrt(float64(sum))).
// Every term is a non-negative integer, so every partial sum the reference forms is one too, none larger than
// S = sum (a_i - b_i)^2.  While S <= 2^24 every f32 add is exact and the value is sqrt_rn(float(S)), a function of S alone
// (u8_value_of_s).  Beyond 2^24 the adds round and the value depends on the chains: u8_chain_sum evaluates them as written.
// What the rounding can do at most: a term passes at most floor(D / 4) + 2 adds of its chain (the first add to 0 is exact, the
// tail adds at most three) and the three final adds, each >= (1 - 2^-24) of the exact sum, so
//   reference sum >= S (1 - 2^-24)^(floor(D / 4) + 5) >= S (1 - (floor(D / 4) + 6) 2^-24)          (u8_value_lower_bound).
// Device-only; the functions compile with fp contraction off.
#pragma once
#include "lb_device.h"

namespace lb {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t U8_EXACT_S = 1u << 24; // S up to here: every f32 add of the reference is exact

// the value of a pair whose exact integer sum is S <= 2^24
__device__ __forceinline__ float u8_value_of_s(uint32_t S) { return (float)sqrt((double)(float)S); }

// The value of a pair whose four exact chain sums S_j = sum over i = j mod 4 of (a_i - b_i)^2 (the tail elements in S_0) are each
// <= 2^24, whatever their total: every partial sum of chain j is an integer no larger than S_j, so every add inside every chain
// is exact and s_j = float(S_j); the three adds of the chains then round as the reference's do.  That is every pair for
// D <= 1032 (258 * 4), and S up to 2^26.  With the total <= 2^24 too the three adds are exact and this is u8_value_of_s(S).
__device__ __forceinline__ float u8_value_of_chains(uint32_t S0, uint32_t S1, uint32_t S2, uint32_t S3)
{
#pragma clang fp contract(off)
    const float sum = (((float)S0 + (float)S1) + (float)S2) + (float)S3;
    return (float)sqrt((double)sum);
}

// a lower bound of the reference value of a pair with the exact sum S (any S): the float nearest the bound above is at most
// the reference's sum, which is a float no smaller than the bound, and sqrt and the roundings are monotone
__device__ __forceinline__ float u8_value_lower_bound(uint32_t S, int D)
{
    const double lb = (double)S * (1.0 - (double)(D / 4 + 6) * 0x1p-24);
    return (float)sqrt((double)(float)lb);
}

// the four bytes of w against q[0 .. 4): one step of the four chains (v_cvt_f32_ubyte0..3, v_sub, v_mul, v_add)
template <class QT>
__device__ __forceinline__ void u8_chain_step(uint32_t w, const QT *q, float &s0, float &s1, float &s2, float &s3)
{
#pragma clang fp contract(off)
    const float d0 = (float)(w & 255u) - (float)q[0];
    const float d1 = (float)((w >> 8) & 255u) - (float)q[1];
    const float d2 = (float)((w >> 16) & 255u) - (float)q[2];
    const float d3 = (float)(w >> 24) - (float)q[3];
    s0 = s0 + d0 * d0;
    s1 = s1 + d1 * d1;
    s2 = s2 + d2 * d2;
    s3 = s3 + d3 * d3;
}

// the reference's f32 sum of one pair, one lane, straight from memory.  QT: the queries' element type, uint8_t or float
// holding uint8 values (the scan reads its queries widened).  ALIGNED16: D % 16 == 0 and x 16-B aligned (16-B row loads).
template <bool ALIGNED16, class QT>
__device__ __forceinline__ float u8_chain_sum(const uint8_t *x, const QT *q, int D)
{
#pragma clang fp contract(off)
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int i = 0;
    if (ALIGNED16) {
        for (; i < D; i += 16) {
            const u32x4 w = *reinterpret_cast<const u32x4 *>(x + i);
            u8_chain_step(w.x, q + i, s0, s1, s2, s3);
            u8_chain_step(w.y, q + i + 4, s0, s1, s2, s3);
            u8_chain_step(w.z, q + i + 8, s0, s1, s2, s3);
            u8_chain_step(w.w, q + i + 12, s0, s1, s2, s3);
        }
    } else {
        for (; i + 4 <= D; i += 4) {
            const uint32_t w = (uint32_t)x[i] | ((uint32_t)x[i + 1] << 8) | ((uint32_t)x[i + 2] << 16) | ((uint32_t)x[i + 3] << 24);
            u8_chain_step(w, q + i, s0, s1, s2, s3);
        }
        for (; i < D; i++) {
            const float d = (float)x[i] - (float)q[i];
            s0 = s0 + d * d;
        }
    }
    return ((s0 + s1) + s2) + s3;
}

// the reported distance of one pair by the chain arithmetic throughout (any D, any alignment)
template <class QT>
__device__ __forceinline__ float u8_pair_distance(const uint8_t *x, const QT *q, int D)
{
    const bool al = D % 16 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const float sum = al ? u8_chain_sum<true>(x, q, D) : u8_chain_sum<false>(x, q, D);
    return (float)sqrt((double)sum);
}

} // namespace lb
