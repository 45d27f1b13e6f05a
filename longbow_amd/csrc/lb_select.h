// lb_select.h -- the one definition of "one workgroup finds the k-th smallest of its unique u64 entries and writes the k
// results": the MSB radix select, the compaction of what lies at or below its pivot, and the result emit.  Used by
// select_kernel / emit_lists_kernel (kernels_select.hip), the finish kernels (kernels_finish.hip) and ivfsq8_select_kernel
// (kernels_ivfsq8.hip: 1024 threads, integer keys, an emit of its own), which differ only in where their entries live (LDS,
// registers, global memory).  ivf_select_kernel (kernels_ivf.hip) takes wave_or_and_u64, the scratch's size and
// allow_big_lds from here and keeps its own text of the walk, for a measured reason given there.
//
// What the shared form does that one of the three earlier copies did not, and why no result moves:
//   - select_kernel's counting passes now skip its kEntryMax padding: the radix path runs only with n > kc real entries, and
//     padding is the largest value, so it lay beyond rank `need` in every pass it was counted in.
//   - select_kernel gets the `diff == 0` return: unreachable there (it comes with at least two unique entries); one compare.
//   - the finish kernels reduce OR / AND by DPP instead of shuffles: the same OR / AND, in lane 63 instead of lane 0.
#pragma once
#include "lb_device.h"

#include <float.h>

namespace lb {

constexpr int SEL_THREADS = 256;

__device__ __forceinline__ uint32_t next_pow2(uint32_t v)
{
    if (v <= 2) return 2;
    return 1u << (32 - __builtin_clz(v - 1));
}

// Kernels that carve more than 64 KB of dynamic LDS must opt in once.
template <typename K>
static void allow_big_lds(K kernel, size_t bytes)
{
    if (bytes > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// In-LDS bitonic sort of P (power of two) u64 keys, ascending, by the whole workgroup.
__device__ __forceinline__ void bitonic_sort_u64(uint64_t *sh, uint32_t P, int tid, int nthreads)
{
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (P >> 1); t += nthreads) {
                const uint32_t i = 2 * t - (t & (j - 1));
                const uint32_t l = i + j;
                const uint64_t a = sh[i], b = sh[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    sh[i] = b;
                    sh[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// lane permutes on the DPP path (no LDS round trip): OR / AND of a u64 over the 64 lanes, result in lane 63
__device__ __forceinline__ void wave_or_and_u64(uint64_t &o, uint64_t &a)
{
#define LB_STEP(CTRL, RM)                 \
    o |= dpp_u64<CTRL, RM>(o);            \
    a &= dpp_u64<CTRL, RM>(a);
    LB_STEP(0xB1, 0xf)  // quad_perm [1,0,3,2]
    LB_STEP(0x4E, 0xf)  // quad_perm [2,3,0,1]
    LB_STEP(0x141, 0xf) // row_half_mirror
    LB_STEP(0x140, 0xf) // row_mirror
    LB_STEP(0x142, 0xa) // row_bcast15 -> rows 1,3 (disabled rows keep their own value: x|x, x&x)
    LB_STEP(0x143, 0xc) // row_bcast31 -> rows 2,3
#undef LB_STEP
}

// LDS scratch of radix_kth.  (The OR / AND pair of its first step lives in bins[0..4): the bins are not in use yet.)
struct alignas(8) RadixScratch {
    uint32_t bins[256];    // one pass' histogram of the byte at `shift`
    uint32_t wave_sum[4];  // the four waves' totals of the scan over the bins
    uint32_t bucket;       // the bin that holds the entry of rank `need`
    uint32_t need;         // its rank within that bin (1-based)
    uint32_t whole_bucket; // the rank is the bin's last: everything in the bin is kept, no further pass
};
// ... and beside it the scalars of the kernels around the selection
struct SelectScratch {
    RadixScratch radix;
    uint32_t out_count;   // compaction counter: entries handed a staging slot
    uint32_t valid_count; // real (non-kEntryMax) entries counted
    uint32_t spare[2];    // (unused: they keep the size at the 256 + 4 + 8 words the launchers have always carved, so that no launch's LDS changes)
};
static_assert(sizeof(SelectScratch) == (256 + 4 + 8) * sizeof(uint32_t), "the launchers' LDS tail");

// MSB radix select, 8 bits a pass: the pivot such that exactly `need` (>= 1) of the entries visited are <= it (entries are
// unique: the row is part of the key).  each(f) calls f(e) for every entry the calling thread owns and skips kEntryMax
// padding where its storage has any.  All NT threads of the workgroup call it; the entries must be visible to them on entry.
template <int NT, typename Each>
__device__ __forceinline__ uint64_t radix_kth(Each each, uint32_t need, RadixScratch &s, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    // Leading bytes shared by every entry (distances live in a narrow range) need no pass.
    unsigned long long *red = reinterpret_cast<unsigned long long *>(s.bins); // [0] = OR, [1] = AND of the entries
    if (tid == 0) { red[0] = 0ull; red[1] = ~0ull; }
    __syncthreads();
    {
        uint64_t o = 0, an = ~0ull;
        each([&](uint64_t e) { o |= e; an &= e; });
        wave_or_and_u64(o, an); // one pair of LDS atomics per wave, not per thread
        if (lane == 63) {
            atomicOr(&red[0], (unsigned long long)o);
            atomicAnd(&red[1], (unsigned long long)an);
        }
    }
    __syncthreads();
    const uint64_t diff = red[0] ^ red[1]; // bit positions that differ among the entries
    const uint64_t common = red[1];
    __syncthreads();
    if (diff == 0ull) return common | 0xffffffffull; // one entry (or none): it is the pivot
    const int same_bytes = __builtin_clzll(diff) >> 3; // whole leading bytes identical
    uint64_t prefix = 0, mask = 0;
    if (same_bytes > 0) {
        mask = ~0ull << (64 - 8 * same_bytes);
        prefix = common & mask;
    }
    const bool binner = NT == 256 || tid < 256; // one thread per bin
    for (int shift = 56 - 8 * same_bytes; shift >= 0; shift -= 8) {
        if (binner) s.bins[tid] = 0;
        __syncthreads();
        each([&](uint64_t e) {
            if ((e & mask) == prefix) atomicAdd(&s.bins[(uint32_t)(e >> shift) & 0xffu], 1u);
        });
        __syncthreads();
        const uint32_t h = binner ? s.bins[tid] : 0u;
        uint32_t incl = wave_incl_scan(h, lane);
        if (binner && lane == 63) s.wave_sum[wave] = incl;
        __syncthreads();
        if (binner) {
            uint32_t base = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) base += (w < wave) ? s.wave_sum[w] : 0u;
            incl += base;
            const uint32_t excl = incl - h;
            if (excl < need && need <= incl) {
                s.bucket = (uint32_t)tid;
                s.need = need - excl;
                s.whole_bucket = (need == incl) ? 1u : 0u;
            }
        }
        __syncthreads();
        prefix |= (uint64_t)s.bucket << shift;
        mask |= 0xffull << shift;
        need = s.need;
        const bool whole_bucket = s.whole_bucket != 0u;
        __syncthreads();
        if (whole_bucket) { // (entries are unique, so the row bytes are rarely ever walked)
            prefix |= ~mask; // every entry sharing the resolved bytes is kept; this bound is >= the wanted entry
            break;
        }
    }
    return prefix; // >= the entry of rank `need` and < the next one
}

// The `keep` entries <= pivot (radix_kth's, so there are exactly `keep`) -> stage[0 .. keep) in no order, stage[keep .. limit)
// = kEntryMax.  *counter is zero on entry; a slot is written only inside the staging area, whatever the pivot.  No barrier
// at the end: the caller syncs before it reads the stage.
// Where the stage is the front of the caller's global list (select_kernel without room in LDS), the pad is written there too:
// list[keep .. limit), which nobody reads (the caller publishes cnt = keep) and which fits (limit = Pk < cap on that path).
template <int NT, typename Each>
__device__ __forceinline__ void compact_le(Each each, uint64_t pivot, uint64_t *stage, uint32_t keep, uint32_t limit,
                                           uint32_t *counter, int tid)
{
    each([&](uint64_t e) {
        if (e <= pivot) {
            const uint32_t pos = atomicAdd(counter, 1u);
            if (pos < limit) stage[pos] = e;
        }
    });
    for (uint32_t i = keep + (uint32_t)tid; i < limit; i += NT) stage[i] = kEntryMax;
}

// The sorted prefix sorted[0 .. nsorted) -> query q's k results; FLT_MAX / -1 beyond it.  ids (or null: the row itself) maps rows to labels.
__device__ __forceinline__ void emit_sorted(const uint64_t *sorted, uint32_t nsorted, int k, int64_t q, const int64_t *ids,
                                            float *out_dist, int64_t *out_labels, int tid, int nthreads)
{
    for (int r = tid; r < k; r += nthreads) {
        float d = FLT_MAX;
        int64_t lab = -1;
        if ((uint32_t)r < nsorted) {
            const uint64_t e = sorted[r];
            d = entry_key(e);
            const uint32_t row = entry_row(e);
            lab = ids ? ids[row] : (int64_t)row;
        }
        out_dist[q * k + r] = d;
        out_labels[q * k + r] = lab;
    }
}

} // namespace lb
