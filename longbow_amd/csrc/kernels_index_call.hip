// kernels_index_call.hip -- the row bitmap given with a search call on the flat index (lb_gpu_index_search*_bitmap*; semantics in
// include/longbow_gpu.h): the call's bits, ANDed with the handle's effective mask, become the view of this call alone -- a byte
// mask and the ascending list of its visible rows, both in the call's workspace -- which every search kernel then takes as the
// values it takes of the handle's view (IndexRowView: mask / rowmap / n).
//
// Three launches on the call's stream, and four bytes (the total) for the host:
//   index_call_bits_kernel     bits AND handle mask -> the call's byte mask, and a count per workgroup of CP-sized block
//   launch_compact_offsets     (kernels_filter.hip) the counts' exclusive prefix in place, the total behind them
//   index_call_scatter_kernel  the call's byte mask -> the ascending row list
// One workgroup of 256 threads per 2,048 positions (kernels_filter.hip's CP_ROWS).  Thread t of block b owns bitmap byte
// b 256 + t, which is exactly its eight rows: the byte loads of a wave are 64 consecutive bytes at any base address.  Integer
// only; no workgroup waits for another; the output depends on the inputs alone.
#include "lb_device.h"
#include "lb_select.h"

namespace lb {

constexpr int IC_THREADS = 256;
constexpr int IC_PER = 8; // rows per thread: one bitmap byte, eight mask bytes
constexpr int IC_ROWS = IC_THREADS * IC_PER;
static_assert(IC_ROWS == INDEX_CALL_BLOCK_ROWS, "lb_device.h names the block for the host's sizes");

// bit i set <=> byte i of v is non-zero
__device__ __forceinline__ uint32_t ic_nonzero_bytes(uint64_t v)
{
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < IC_PER; i++) bits |= ((v >> (8 * i)) & 0xffull) ? (1u << i) : 0u;
    return bits;
}

// Every load is issued whether or not its value is wanted, at an address clamped into the array, and masked afterwards (a load
// inside a divergent branch is waited for before the branch ends).  Only the handle mask's last, partial group of eight -- one
// thread of the whole grid -- takes loads a byte.
// bits: [ceil(n / 8)] bytes at any address; hmask: the handle's effective mask, [n] bytes, 8-byte aligned, or null; cmask: the
// call's mask, whole blocks of IC_ROWS bytes (rows >= n come out 0); counts[b]: rows block b leaves visible.  n >= 1.
__global__ __launch_bounds__(IC_THREADS) void index_call_bits_kernel(const uint8_t *bits, const uint8_t *hmask, int64_t n, uint8_t *cmask,
                                                                      uint32_t *counts)
{
    __shared__ uint32_t s_wave[IC_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t byte = (int64_t)blockIdx.x * IC_THREADS + tid; // this thread's bitmap byte
    const int64_t base = byte * IC_PER;                          // and its first row
    const int64_t nbytes = (n + 7) >> 3, full = n & ~(int64_t)7; // rows [0, full) lie in whole groups of eight
    uint32_t keep = bits[byte < nbytes ? byte : nbytes - 1];
    // rows of this group that exist: all eight, the first n % 8 of the last byte, none behind it
    const uint32_t exist = base + IC_PER <= n ? 0xffu : base < n ? (1u << (uint32_t)(n - base)) - 1u : 0u;
    keep &= exist;
    if (hmask) {
        uint64_t v = 0;
        if (full > 0) v = *reinterpret_cast<const uint64_t *>(hmask + (base < full ? base : full - IC_PER));
        uint32_t nz = ic_nonzero_bytes(v);
        if (base == full && full < n) { // the partial group
            nz = 0;
            for (int i = 0; i < IC_PER; i++)
                if (base + i < n && hmask[base + i]) nz |= 1u << i;
        }
        keep &= nz;
    }
    uint64_t out = 0;
#pragma unroll
    for (int i = 0; i < IC_PER; i++) out |= (uint64_t)((keep >> i) & 1u) << (8 * i);
    *reinterpret_cast<uint64_t *>(cmask + base) = out;
    uint32_t c = (uint32_t)__popc(keep);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if (lane == 0) s_wave[wave] = c;
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// cmask as index_call_bits_kernel left it (whole blocks, 0 / 1 bytes), offsets: the counts' exclusive prefix; rowmap: the rows
// whose byte is set, ascending
__global__ __launch_bounds__(IC_THREADS) void index_call_scatter_kernel(const uint8_t *cmask, const uint32_t *offsets, uint32_t *rowmap)
{
    __shared__ uint32_t s_wave[IC_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = ((int64_t)blockIdx.x * IC_THREADS + tid) * IC_PER;
    const uint32_t keep = ic_nonzero_bytes(*reinterpret_cast<const uint64_t *>(cmask + base));
    const uint32_t c = (uint32_t)__popc(keep);
    const uint32_t incl = wave_incl_scan(c, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < IC_THREADS / 64; w++)
        if (w < wave) before += s_wave[w];
    uint32_t at = offsets[blockIdx.x] + before + incl - c;
#pragma unroll
    for (int i = 0; i < IC_PER; i++)
        if ((keep >> i) & 1u) rowmap[at++] = (uint32_t)(base + i);
}

void launch_index_call_bits(const uint8_t *d_bits, const uint8_t *hmask, int64_t n, uint8_t *cmask, uint32_t *scratch, hipStream_t s)
{
    const int64_t nb = (n + IC_ROWS - 1) / IC_ROWS;
    if (nb <= 0) return;
    hipLaunchKernelGGL(index_call_bits_kernel, dim3((unsigned)nb), dim3(IC_THREADS), 0, s, d_bits, hmask, n, cmask, scratch);
}

void launch_index_call_scatter(const uint8_t *cmask, int64_t n, const uint32_t *scratch, uint32_t *rowmap, hipStream_t s)
{
    const int64_t nb = (n + IC_ROWS - 1) / IC_ROWS;
    if (nb <= 0) return;
    hipLaunchKernelGGL(index_call_scatter_kernel, dim3((unsigned)nb), dim3(IC_THREADS), 0, s, cmask, scratch, rowmap);
}

} // namespace lb
