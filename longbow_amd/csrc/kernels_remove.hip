// kernels_remove.hip -- removal and compaction of the flat index (index_remove.hip; semantics in include/longbow_gpu.h:
// lb_gpu_index_remove*, lb_gpu_index_compact).
//
// Removal clears a row's byte in two per-row byte arrays, `live` (non-zero = live) and the index's effective mask, and counts
// the rows that were live before the call.  By position one lane takes one entry of the caller's list, and a row named twice
// must count once: the live byte is cleared by an atomic AND on the word that holds it, whose returned old value tells exactly
// one of the lanes that it was the one.  By id one lane takes one ROW, so nothing races: it reads the row's id (coalesced 8-byte
// reads) and looks it up in the sorted set by binary search, the set in LDS when it fits.  Either way a wave counts by ballot
// and a workgroup adds once.
//
// Compaction gathers rows through the ascending list of survivors into a scratch that does not overlap the source; the host
// (index_remove.hip) walks rounds and copies each back, which is what makes the whole in place.  Pure HBM-bound copies: the
// widest piece the row size allows per lane (16 bytes for every f32 / fp16 dimension that is a multiple of 4 / 8), a grid of a
// few workgroups per CU that strides over the rows.
#include "lb_device.h"

namespace lb {

constexpr int RM_THREADS = 256;
constexpr int RM_SET_LDS = 4096; // ids of the set kept in LDS (32 KiB)

// the workgroup's count into *removed: ballot per wave, one LDS add per wave, one global add per workgroup
__device__ __forceinline__ void rm_count(bool hit, uint32_t *s_cnt, uint32_t *removed)
{
    const uint32_t c = (uint32_t)__popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(s_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0 && *s_cnt) atomicAdd(removed, *s_cnt);
}

__global__ __launch_bounds__(RM_THREADS) void remove_rows_kernel(const int64_t *rows, int64_t cnt, int64_t ntotal, uint32_t *live_words,
                                                                 uint8_t *mask, uint32_t *removed)
{
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x; // (the grid covers cnt: one entry per lane)
    bool hit = false;
    if (i < cnt) {
        const int64_t r = rows[i];
        if (r >= 0 && r < ntotal) {
            const uint32_t byte = 0xffu << (8 * (uint32_t)(r & 3));
            const uint32_t old = atomicAnd(live_words + (r >> 2), ~byte);
            hit = (old & byte) != 0;
            if (hit) mask[r] = 0;
        }
    }
    rm_count(hit, &s_cnt, removed);
}

// IN_LDS: the whole set is staged in LDS (nset <= RM_SET_LDS)
template <bool IN_LDS>
__global__ __launch_bounds__(RM_THREADS) void remove_ids_kernel(const int64_t *ids, int64_t ntotal, const int64_t *set, int64_t nset,
                                                                uint8_t *live, uint8_t *mask, uint32_t *removed)
{
    __shared__ uint32_t s_cnt;
    __shared__ int64_t s_set[IN_LDS ? RM_SET_LDS : 1];
    if (threadIdx.x == 0) s_cnt = 0;
    if (IN_LDS)
        for (int64_t i = threadIdx.x; i < nset; i += RM_THREADS) s_set[i] = set[i];
    __syncthreads();
    const int64_t *tab = IN_LDS ? s_set : set;
    uint32_t mine = 0;
    for (int64_t r = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x; r < ntotal; r += (int64_t)gridDim.x * RM_THREADS) {
        if (!live[r]) continue;
        const int64_t id = ids[r];
        int64_t lo = 0, hi = nset; // first entry >= id
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (tab[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        if (lo < nset && tab[lo] == id) {
            live[r] = 0;
            mask[r] = 0;
            mine++;
        }
    }
    // (lanes differ in their trip counts: the per-lane sums are added by the wave once the loop is over)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(removed, s_cnt);
}

__global__ __launch_bounds__(RM_THREADS) void first_dead_kernel(const uint8_t *live, int64_t ntotal, uint32_t *out)
{
    uint32_t first = 0xffffffffu;
    for (int64_t r = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x; r < ntotal; r += (int64_t)gridDim.x * RM_THREADS)
        if (!live[r]) { first = (uint32_t)r; break; } // (a lane's rows ascend: its first is its smallest)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(first, off);
        first = o < first ? o : first;
    }
    if ((threadIdx.x & 63) == 0 && first != 0xffffffffu) atomicMin(out, first);
}

// Row j of the destination = row map[j] of the source, rows of ppr pieces of sizeof(T) bytes.  2^lg lanes share a row (the
// smallest power of two that covers ppr, at most the workgroup), so that a lane finds its row and piece by shifts.
template <typename T>
__global__ __launch_bounds__(RM_THREADS) void gather_rows_kernel(const T *src, const uint32_t *map, int64_t cnt, uint32_t ppr, int lg, T *dst)
{
    const uint32_t sub = threadIdx.x & ((1u << lg) - 1u);
    const int64_t rpb = RM_THREADS >> lg; // rows per workgroup and step
    for (int64_t j = (int64_t)blockIdx.x * rpb + (threadIdx.x >> lg); j < cnt; j += (int64_t)gridDim.x * rpb) {
        const T *from = src + (int64_t)map[j] * ppr;
        T *to = dst + j * (int64_t)ppr;
        for (uint32_t p = sub; p < ppr; p += 1u << lg) to[p] = from[p];
    }
}

static unsigned rm_grid(int64_t work, int device)
{
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        cus = 256;
    }
    int64_t blocks = (work + RM_THREADS - 1) / RM_THREADS;
    if (blocks > (int64_t)cus * 8) blocks = (int64_t)cus * 8;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

void launch_remove_rows(const int64_t *rows, int64_t cnt, int64_t ntotal, uint8_t *live, uint8_t *mask, uint32_t *removed, hipStream_t s)
{
    if (cnt <= 0 || ntotal <= 0) return;
    hipLaunchKernelGGL(remove_rows_kernel, dim3((unsigned)((cnt + RM_THREADS - 1) / RM_THREADS)), dim3(RM_THREADS), 0, s, rows, cnt, ntotal,
                       reinterpret_cast<uint32_t *>(live), mask, removed);
}

void launch_remove_ids(const int64_t *ids, int64_t ntotal, const int64_t *set, int64_t nset, uint8_t *live, uint8_t *mask,
                       uint32_t *removed, hipStream_t s)
{
    if (nset <= 0 || ntotal <= 0) return;
    int device = 0;
    (void)hipGetDevice(&device);
    const dim3 grid(rm_grid(ntotal, device));
    if (nset <= RM_SET_LDS)
        hipLaunchKernelGGL(remove_ids_kernel<true>, grid, dim3(RM_THREADS), 0, s, ids, ntotal, set, nset, live, mask, removed);
    else
        hipLaunchKernelGGL(remove_ids_kernel<false>, grid, dim3(RM_THREADS), 0, s, ids, ntotal, set, nset, live, mask, removed);
}

void launch_first_dead(const uint8_t *live, int64_t ntotal, uint32_t *out, hipStream_t s)
{
    if (ntotal <= 0) return;
    int device = 0;
    (void)hipGetDevice(&device);
    hipLaunchKernelGGL(first_dead_kernel, dim3(rm_grid(ntotal, device)), dim3(RM_THREADS), 0, s, live, ntotal, out);
}

void launch_gather_rows(const void *src, const uint32_t *map, int64_t cnt, size_t row_bytes, void *dst, int device, hipStream_t s)
{
    if (cnt <= 0 || row_bytes == 0) return;
    // the widest piece that divides the row and that both bases are aligned to: every row then starts on a piece boundary
    const uintptr_t bits = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)row_bytes;
    auto go = [&](auto zero) {
        using T = decltype(zero);
        const uint32_t ppr = (uint32_t)(row_bytes / sizeof(T));
        int lg = 0;
        while (lg < 8 && (1u << lg) < ppr) lg++;
        hipLaunchKernelGGL(gather_rows_kernel<T>, dim3(rm_grid(cnt << lg, device)), dim3(RM_THREADS), 0, s, static_cast<const T *>(src), map,
                           cnt, ppr, lg, static_cast<T *>(dst));
    };
    if ((bits & 15) == 0) go(uint4{});
    else if ((bits & 7) == 0) go(uint64_t{});
    else if ((bits & 3) == 0) go(uint32_t{});
    else go(uint8_t{});
}

} // namespace lb
