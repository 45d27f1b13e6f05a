// kernels_select.hip -- batched top-k selection and cross-shard merge (the exact re-rank + proof: kernels_finish.hip).
//
// select:  per query, bitonic-sort the admitted (key,row) entries in LDS, keep the best kc,
//          publish the kc-th entry as the next admission threshold.  The ordering it realises
//          is the canonical form of BruteForceIndex.SearchVectors' bounded heap
//          (internal/store/adaptive_index.go:176-222): ascending (distance, row position).
// merge:   store.MergeSortedStreams (internal/store/result_merger.go:34-101) for S shards.
#include "lb_device.h"
#include "lb_select.h"

#include <float.h>
#include <algorithm>

#pragma clang fp contract(off)

namespace lb {

__global__ void init_cand_kernel(CandState cs, const int *qsel, int nsel)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nsel) {
        const int i = qsel ? qsel[j] : j;
        cs.cnt[i] = 0;
        cs.tau[i] = kEntryMax;
        cs.flags[i] = 0;
    }
}

void launch_init_cand(CandState cs, const int *qsel, int nsel, hipStream_t s)
{
    if (nsel <= 0) return;
    hipLaunchKernelGGL(init_cand_kernel, dim3((nsel + 255) / 256), dim3(256), 0, s, cs, qsel, nsel);
}

// ---------------------------------------------------------------------------
// select: keep the kc smallest of n unique u64 entries, sorted.
//   n <= 2*kc : bitonic sort of everything.
//   otherwise : MSB radix select (8 passes of 8 bits over the LDS copy) finds the kc-th smallest
//               entry exactly (entries are unique: the row is part of the key), the <= pivot
//               entries are compacted and only those kc are sorted (lb_select.h: radix_kth, compact_le).
// LDS: entries u64[next_pow2(cap)] | SelectScratch
template <int NT> // threads per workgroup: 256 (throughput, many queries) or 1024 (latency, few queries)
__global__ __launch_bounds__(NT) void select_kernel(CandState cs, const int *qsel, int kc,
                                                             uint32_t boot_rows, uint32_t need_at_least,
                                                             EmitArgs em, uint32_t striped, uint32_t unsorted)
{
    // need_at_least: a list shorter than this means a sampled threshold admitted too few rows -> flag bit 2,
    // the query is redone without sampling.
    extern __shared__ __attribute__((aligned(16))) uint64_t sh[];
    const int q = qsel ? qsel[blockIdx.x] : blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // boot_rows > 0: the bootstrap chunk stored one entry per row without atomics
    // striped: positions s, s+16, ... of the list were handed out by 16 counters (slot = blockIdx.x);
    // the list then has holes, which are read as kEntryMax exactly like masked rows of a bootstrap chunk
    uint32_t my_stripe_cnt = 0;
    if (striped) {
        __shared__ uint32_t s_stripe[LB_STRIPES];
        if (tid < LB_STRIPES) s_stripe[tid] = cs.stripes[(blockIdx.x * LB_STRIPES + tid) * LB_STRIPE_PAD];
        __syncthreads();
        uint32_t mx = 0;
#pragma unroll
        for (int st = 0; st < LB_STRIPES; st++) mx = s_stripe[st] > mx ? s_stripe[st] : mx;
        my_stripe_cnt = s_stripe[tid & (LB_STRIPES - 1)];
        boot_rows = mx * LB_STRIPES; // (0 admissions -> the plain path below sees cnt[q] == 0)
    }
    const uint32_t raw = boot_rows ? boot_rows : cs.cnt[q];
    uint32_t n = raw < cs.cap ? raw : cs.cap;
    uint64_t *list = cs.lists + (size_t)q * cs.cap;
    if (raw > cs.cap && tid == 0) atomicOr(&cs.flags[q], 1u);
    // last select of a scan-path search: write the k results (and the slot's status word, to pinned host
    // memory) from the sorted prefix sorted[0..nsorted) instead of launching emit_lists_kernel
    auto emit = [&](const uint64_t *sorted, uint32_t nsorted) {
        if (em.out_dist == nullptr) return;
        emit_sorted(sorted, nsorted, em.k, q, em.ids, em.out_dist, em.out_labels, tid, NT);
        if (em.flags_host && tid == 0) em.flags_host[q] = atomicOr(&cs.flags[q], 0u);
    };
    if (n == 0) {
        if (tid == 0) {
            cs.tau[q] = kEntryMax;
            cs.cnt[q] = 0;
            if (need_at_least) atomicOr(&cs.flags[q], 4u);
        }
        emit(nullptr, 0);
        return;
    }
    const uint32_t P = next_pow2(n);
    SelectScratch &ss = *reinterpret_cast<SelectScratch *>(sh + next_pow2(cs.cap));

    if (tid == 0) { ss.out_count = 0; ss.valid_count = 0; }
    uint32_t myvalid = 0;
    for (uint32_t i = tid; i < P; i += NT) { // (NT is a multiple of 16: a thread stays in one stripe)
        const bool there = i < n && (!striped || (i / LB_STRIPES) < my_stripe_cnt);
        const uint64_t e = there ? list[i] : kEntryMax;
        sh[i] = e;
        myvalid += (e != kEntryMax) ? 1u : 0u;
    }
    __syncthreads();
    if (boot_rows) { // masked-out rows of the bootstrap chunk hold kEntryMax: count the real ones
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) myvalid += __shfl_xor(myvalid, off); // one LDS atomic per wave
        if (lane == 0 && myvalid) atomicAdd(&ss.valid_count, myvalid);
        __syncthreads();
        n = ss.valid_count;
        __syncthreads();
        if (n == 0) {
            if (tid == 0) {
                cs.tau[q] = kEntryMax;
                cs.cnt[q] = 0;
                if (need_at_least) atomicOr(&cs.flags[q], 4u);
            }
            emit(nullptr, 0);
            return;
        }
    }
    const uint32_t keep = n < (uint32_t)kc ? n : (uint32_t)kc;
    if (n < need_at_least && tid == 0) atomicOr(&cs.flags[q], 4u);

    if (P <= 2u * next_pow2((uint32_t)kc) || n <= (uint32_t)kc) {
        bitonic_sort_u64(sh, P, tid, NT); // kEntryMax padding sorts last
        for (uint32_t i = tid; i < keep; i += NT) list[i] = sh[i];
        if (tid == 0) {
            cs.cnt[q] = keep;
            cs.tau[q] = n >= (uint32_t)kc ? sh[kc - 1] : kEntryMax;
        }
        emit(sh, keep);
        return;
    }

    // ---- radix select of the kc-th smallest, over the LDS copy (its padding and holes are not entries) ----
    auto each = [&](auto f) {
        for (uint32_t i = tid; i < P; i += NT) {
            const uint64_t e = sh[i];
            if (e != kEntryMax) f(e);
        }
    };
    const uint64_t pivot = radix_kth<NT>(each, (uint32_t)kc, ss.radix, tid); // exactly kc entries are <= pivot
    // compact the kc entries <= pivot (unordered), then sort them.  The staging area is the unused tail of
    // the LDS entry array when there is room, else the front of the global list.
    const uint32_t Pk = next_pow2((uint32_t)kc);
    uint64_t *stage = (P + Pk <= next_pow2(cs.cap)) ? sh + P : list;
    compact_le<NT>(each, pivot, stage, (uint32_t)kc, Pk, &ss.out_count, tid);
    __syncthreads();
    if (unsorted) {
        // the caller re-ranks the kept entries anyway and only needs to know which one has the worst key: it goes to
        // position kc - 1 (one swap), the other kc - 1 stay as the compaction left them -- no sort (-4 us)
        unsigned long long *mx = reinterpret_cast<unsigned long long *>(ss.radix.bins);
        if (tid == 0) mx[0] = 0ull;
        __syncthreads();
        unsigned long long m = 0ull;
        for (uint32_t i = tid; i < (uint32_t)kc; i += NT) m = stage[i] > m ? stage[i] : m;
        if (m) atomicMax(&mx[0], m);
        __syncthreads();
        const uint64_t worst = mx[0];
        __syncthreads();
        for (uint32_t i = tid; i < (uint32_t)kc; i += NT) {
            const uint64_t e = stage[i];
            if (e == worst && i != (uint32_t)kc - 1) { // entries are unique: one thread swaps
                stage[i] = stage[kc - 1];
                stage[kc - 1] = e;
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < (uint32_t)kc; i += NT) list[i] = stage[i];
        if (tid == 0) {
            cs.cnt[q] = (uint32_t)kc;
            cs.tau[q] = pivot;
        }
        return; // (no emit on this route: the re-rank writes the results)
    }
    // (this path has P > 2 * Pk, so sh[0..Pk) and the staging tail sh[P..P+Pk) do not overlap)
    for (uint32_t i = tid; i < Pk; i += NT) sh[i] = stage[i];
    __syncthreads();
    bitonic_sort_u64(sh, Pk, tid, NT);
    for (uint32_t i = tid; i < (uint32_t)kc; i += NT) list[i] = sh[i];
    if (tid == 0) {
        cs.cnt[q] = (uint32_t)kc;
        cs.tau[q] = pivot;
    }
    emit(sh, (uint32_t)kc);
}

// smap[i] = corpus row behind the i-th of `count` evenly spaced positions of [0, span)
__global__ __launch_bounds__(256) void sample_map_kernel(const uint32_t *rowmap, int64_t span, uint32_t count,
                                                         uint32_t *smap)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const int64_t pos = (int64_t)(((uint64_t)i * (uint64_t)span) / count); // i, span < 2^32
    smap[i] = rowmap ? rowmap[pos] : (uint32_t)pos;
}

void launch_sample_map(const uint32_t *rowmap, int64_t span, uint32_t count, uint32_t *smap, hipStream_t s)
{
    if (count == 0) return;
    hipLaunchKernelGGL(sample_map_kernel, dim3((count + 255) / 256), dim3(256), 0, s, rowmap, span, count, smap);
}

void launch_select(CandState cs, const int *qsel, int nsel, int kc, uint32_t boot_rows, hipStream_t s,
                   uint32_t need_at_least, const EmitArgs *emit, bool striped, bool unsorted)
{
    EmitArgs em{};
    if (emit) em = *emit;
    if (nsel <= 0) return;
    const size_t shmem = (size_t)next_pow2_host(cs.cap) * sizeof(uint64_t) + sizeof(SelectScratch);
    static const int big_max = lb_tunable("LB_SELECT_BIG_MAXQ", 512); // (1024-thread selects: 10 us less than 256-thread ones at 128-384 queries)
    if (nsel <= big_max) { // few queries: one big workgroup each, latency matters
        allow_big_lds(select_kernel<1024>, shmem);
        hipLaunchKernelGGL(select_kernel<1024>, dim3(nsel), dim3(1024), shmem, s, cs, qsel, kc, boot_rows,
                           need_at_least, em,
                           (striped && cs.stripes) ? 1u : 0u, (unsorted && emit == nullptr) ? 1u : 0u);
    } else {
        allow_big_lds(select_kernel<256>, shmem);
        hipLaunchKernelGGL(select_kernel<256>, dim3(nsel), dim3(256), shmem, s, cs, qsel, kc, boot_rows,
                           need_at_least, em,
                           (striped && cs.stripes) ? 1u : 0u, (unsorted && emit == nullptr) ? 1u : 0u);
    }
}

// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// scan path: lists already hold exact distances, sorted by the last select.
__global__ void emit_lists_kernel(CandState cs, const int *qsel, int nsel, int k, const int64_t *ids,
                                  float *out_dist, int64_t *out_labels, uint32_t *flags_host)
{
    const int j = blockIdx.x;
    if (j >= nsel) return;
    const int q = qsel ? qsel[j] : j;
    // the slot's status word goes straight to pinned host memory: no separate D2H copy after the search
    if (flags_host && threadIdx.x == 0) flags_host[q] = cs.flags[q];
    emit_sorted(cs.lists + (size_t)q * cs.cap, cs.cnt[q], k, q, ids, out_dist, out_labels, threadIdx.x, blockDim.x);
}

void launch_emit_lists(CandState cs, const int *qsel, int nsel, int k, const int64_t *ids,
                       float *out_dist, int64_t *out_labels, uint32_t *flags_host, hipStream_t s)
{
    if (nsel <= 0) return;
    hipLaunchKernelGGL(emit_lists_kernel, dim3(nsel), dim3(128), 0, s, cs, qsel, nsel, k, ids, out_dist,
                       out_labels, flags_host);
}

// ---------------------------------------------------------------------------
// Cross-shard merge: per query S*k (dist,label) pairs -> k smallest by (dist, label).
// The LDS sort runs on ONE u64 per entry, (canonical sortable distance << 32) | input index, so 16384
// entries (k = 2048 on 8 shards) fit in 128 KB; labels stay in HBM and are fetched for the k winners.
// Canonical order as in the single-shard lists: every NaN after +inf, padding (label < 0) last of all.
// The index tie-break is (shard, position); entries with EQUAL distances are then re-ranked by label
// (unsigned, so that padding stays last) in a fix-up pass that only touches runs of equal distance.
__global__ __launch_bounds__(SEL_THREADS) void merge_topk_kernel(int nshards, int64_t nq, int k,
                                                                 const float *dist_in,
                                                                 const int64_t *lab_in,
                                                                 int64_t dist_stride, int64_t lab_stride,
                                                                 float *dist_out, int64_t *lab_out)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t mkey[];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t n = (uint32_t)(nshards * k);
    const uint32_t P = next_pow2(n);
    auto label_of = [&](uint32_t idx) -> uint64_t {
        const uint32_t s = idx / (uint32_t)k, r = idx % (uint32_t)k;
        return (uint64_t)lab_in[(int64_t)s * lab_stride + q * k + r];
    };
    for (uint32_t i = tid; i < P; i += SEL_THREADS) {
        uint64_t e = kEntryMax;
        if (i < n) {
            const uint32_t s = i / (uint32_t)k, r = i % (uint32_t)k;
            const int64_t off = q * k + r; // within one shard's [nq][k] block
            const float d = dist_in[(int64_t)s * dist_stride + off] + 0.0f; // -0 -> +0
            const int64_t lab = lab_in[(int64_t)s * lab_stride + off];
            uint32_t sk = (d != d) ? 0xffc00000u : f32_sortable(d);
            if (lab < 0) sk = 0xffffffffu; // padding sorts after every real row, non-finite ones included
            e = ((uint64_t)sk << 32) | i;
        }
        mkey[i] = e;
    }
    __syncthreads();
    bitonic_sort_u64(mkey, P, tid, SEL_THREADS);
    // fix-up + output: an entry inside a run of equal distances moves to its label rank within the run
    for (uint32_t i = tid; i < n; i += SEL_THREADS) {
        const uint64_t e = mkey[i];
        const uint32_t sk = (uint32_t)(e >> 32);
        uint32_t lo = i, hi = i + 1;
        while (lo > 0 && (uint32_t)(mkey[lo - 1] >> 32) == sk) lo--;
        if (lo >= (uint32_t)k) continue; // the whole run lies beyond the output
        while (hi < n && (uint32_t)(mkey[hi] >> 32) == sk) hi++;
        uint32_t pos = i;
        const uint64_t mylab = label_of((uint32_t)e);
        if (hi - lo > 1) {
            pos = lo;
            for (uint32_t j = lo; j < hi; j++) {
                if (j == i) continue;
                const uint64_t lj = label_of((uint32_t)mkey[j]);
                pos += (lj < mylab || (lj == mylab && j < i)) ? 1u : 0u;
            }
        }
        if (pos < (uint32_t)k) {
            const bool pad = sk == 0xffffffffu;
            dist_out[q * k + pos] = pad ? FLT_MAX : sortable_f32(sk);
            lab_out[q * k + pos] = pad ? (int64_t)-1 : (int64_t)mylab;
        }
    }
    // fewer than k inputs in total (never with nshards >= 1, kept for safety)
    for (uint32_t r = n + tid; r < (uint32_t)k; r += SEL_THREADS) {
        dist_out[q * k + r] = FLT_MAX;
        lab_out[q * k + r] = -1;
    }
}

void launch_merge_topk(int nshards, int64_t nq, int k, const float *dist_in, const int64_t *lab_in,
                       int64_t dist_stride, int64_t lab_stride, float *dist_out, int64_t *lab_out, hipStream_t s)
{
    if (nq <= 0 || k <= 0) return;
    const size_t P = next_pow2_host((uint32_t)(nshards * k));
    const size_t shmem = P * sizeof(uint64_t);
    allow_big_lds(merge_topk_kernel, shmem);
    hipLaunchKernelGGL(merge_topk_kernel, dim3((unsigned)nq), dim3(SEL_THREADS), shmem, s, nshards, nq,
                       k, dist_in, lab_in, dist_stride, lab_stride, dist_out, lab_out);
}

} // namespace lb
