// lb_admit.h -- the parts of the candidate kernels' admission epilogue (kernels_gemm*.hip) that are the same in every one-tile
// form: the candidate key, the per-lane threshold, the tile's per-row side inputs, the exact admission rule, and the
// workgroup-local admission list with its flush.  The re-rank's containment proof relies on what is here: every entry that
// passes its query's threshold reaches the query's list, or pushes the query's count past cap, which the select reports as
// an overflow.  (The persistent fp16 forms keep their one-operation keys and per-wave segments in kernels_gemm_tall16.hip.)
#pragma once
#include "lb_device.h"

namespace lb {

// ---- keys -----------------------------------------------------------------------------------------------------------------
// candidate key of (row, query) from their inner product and the row's side input: L2 ||x||^2 - 2 q.x (aux = ||x||^2),
// cosine -q.x / ||x|| (aux = 1 / ||x||), dot -q.x
template <int METRIC>
__device__ __forceinline__ float cand_key(float dot, float aux)
{
    if (METRIC == METRIC_L2) return fmaf(-2.0f, dot, aux);
    if (METRIC == METRIC_COS) return -dot * aux;
    return -dot;
}

// ---- thresholds -----------------------------------------------------------------------------------------------------------
// the admission threshold of query qj: tau_q[qj] (CandState::tau), or 0 -- whose key is NaN: nothing passes -- for a query beyond nq and when
// `none` (a bootstrap or sample pass, or a threshold that arrives later)
__device__ __forceinline__ uint64_t lane_tau(const uint64_t *tau_q, int qj, int nq, bool none)
{
    uint64_t tau = none ? 0ull : tau_q[qj < nq ? qj : nq - 1];
    if (qj >= nq) tau = 0ull;
    return tau;
}
// ---- the tile's per-row side inputs (one-tile forms) ----------------------------------------------------------------------
// Fetched at kernel entry, behind the first stage's requests (one row per thread), and kept in LDS for the epilogue: a load
// per element inside the admission loop would serialise the lane's L2 round trips.  (The helpers take pointers, not a
// reference to the kernel's arguments, which reorders the kernels' code; the mask byte stays at the call site: read through
// a helper, its branch reorders the prologue.)
template <int METRIC>
__device__ __forceinline__ float side_aux(const float *norm2, const float *rnorm, int64_t ri) // the row's side input of cand_key
{
    return METRIC == METRIC_L2 ? norm2[ri] : (METRIC == METRIC_COS ? rnorm[ri] : 0.f);
}
// side inputs of tile rows lr .. lr + 3 (lr a multiple of 4) from the tile's LDS arrays; returns their visibility as 4 bits
// (bit e: row lr + e is in range and not masked out)
__device__ __forceinline__ uint32_t tile_rows4(const float *s_aux, const uint32_t *s_rowid, const uint8_t *s_vis, int lr,
                                               float (&aux)[4], uint32_t (&rid)[4])
{
    const f32x4 av = *reinterpret_cast<const f32x4 *>(&s_aux[lr]);
    const uint4 rv = *reinterpret_cast<const uint4 *>(&s_rowid[lr]);
    const uint32_t vv = *reinterpret_cast<const uint32_t *>(&s_vis[lr]); // 4 bytes of 0/1
    aux[0] = av.x; aux[1] = av.y; aux[2] = av.z; aux[3] = av.w;
    rid[0] = rv.x; rid[1] = rv.y; rid[2] = rv.z; rid[3] = rv.w;
    return (vv & 1u) | ((vv >> 7) & 2u) | ((vv >> 14) & 4u) | ((vv >> 21) & 8u);
}

// ---- admission -------------------------------------------------------------------------------------------------------------
// Exact rule: entry < tau  <=>  key < tau_key, or equal keys and a lower row.  (Float compares treat -0 == +0, matching the
// +0-canonical packed keys; a NaN threshold admits nothing.)
__device__ __forceinline__ uint32_t admit_exact(float key, uint32_t ri, float tk, uint32_t tr)
{
    return (uint32_t)(key < tk) | ((uint32_t)(key == tk) & (uint32_t)(ri < tr));
}
// ---- appending to the per-query lists -------------------------------------------------------------------------------------
// Workgroup-local admission list of the one-tile forms: admissions go to LDS first (two LDS atomics per lane with any) and out
// at the end of the tile with ONE returning global atomic per query of the tile, all in flight at once.  Carved by the kernel
// from LDS that is free by the epilogue: 1 + 2 NQ counters, and FL_CAP entries followed by their query and rank arrays.
// The kernel appends to it (cnt, qcnt, ent, q, rk) between a barrier behind reset() and flush(), which every thread calls.
template <int FL_CAP, int NQ, int NTHREADS>
struct LocalList {
    static constexpr int CAP = FL_CAP;
    uint32_t *cnt;   // entries in the list
    uint32_t *qcnt;  // [NQ] of them per query of the tile ...
    uint32_t *qbase; // [NQ] ... and where they start in the query's list
    uint64_t *ent;   // [FL_CAP]
    uint16_t *q;     // [FL_CAP] query of the entry (in the tile)
    uint16_t *rk;    // [FL_CAP] rank of the entry among its query's
    __device__ __forceinline__ LocalList(uint32_t *counters, uint64_t *entries)
        : cnt(counters), qcnt(counters + 1), qbase(counters + 1 + NQ), ent(entries),
          q(reinterpret_cast<uint16_t *>(entries + FL_CAP)), rk(reinterpret_cast<uint16_t *>(entries + FL_CAP) + FL_CAP)
    {
    }
    __device__ __forceinline__ void reset(int tid) const
    {
        if (tid == 0) *cnt = 0;
        if (tid < NQ) qcnt[tid] = 0;
    }
    // a lane's n entries from position lp on did not fit: mark the reserved positions that exist as unused (flush() skips
    // them; the lane appends to its query's list directly)
    __device__ __forceinline__ void reserved_unused(uint32_t lp, uint32_t n) const
    {
        for (uint32_t i = lp; i < lp + n && i < (uint32_t)FL_CAP; i++) ent[i] = kEntryMax;
    }
    __device__ __forceinline__ void flush(int tid, CandState cs, int q0) const
    {
        __syncthreads();
        if (tid < NQ) {
            const uint32_t n = qcnt[tid];
            qbase[tid] = n ? atomicAdd(&cs.cnt[q0 + tid], n) : 0u; // (n != 0 implies a real query)
        }
        __syncthreads();
        const uint32_t total = *cnt < (uint32_t)FL_CAP ? *cnt : (uint32_t)FL_CAP;
        for (uint32_t i = tid; i < total; i += NTHREADS) {
            const uint64_t e = ent[i];
            if (e == kEntryMax) continue;
            const int ql = (int)q[i];
            const uint32_t pos = qbase[ql] + (uint32_t)rk[i];
            if (pos < cs.cap) cs.lists[(size_t)(q0 + ql) * cs.cap + pos] = e;
        }
    }
};

} // namespace lb
