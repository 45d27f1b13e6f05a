// lb_ivf_u8.h -- what ivf.hip (host) and kernels_ivf_u8.hip (device) share for an IVF-Flat handle whose rows are uint8
// (lb_gpu_ivf_new_u8): the argument block of the list scan and its launcher.  The plan of a batch, the probes and the selection
// are the f32 handle's (lb_ivf.h): IvfBatch is taken as it is, and the scan's own fields lie beside it here, as in lb_ivf_i8.h.
#pragma once
#include "lb_ivf.h"

namespace lb {

// One batch of queries as the uint8 list scan takes it (by value).  b.X and b.Q are not read: b.Q is the batch's queries widened
// to f32, which the coarse index probes with; the scan reads the uint8 queries themselves.
struct IvfU8Scan {
    IvfBatch b;       // D, L, nq, probes, np, seg, keys, pmax
    const uint8_t *X; // [n][D] rows in insertion order
    const uint8_t *Q; // [nq][D] the batch's queries
};

// launch_ivf_scan over uint8 rows and uint8 queries: keys[q][seg[q][p] + i] = entry of the i-th row of the p-th probed list, the
// distance being the flat uint8 index's (kernels_u8.hip; lb_u8_exact.h), bit for bit.  Euclidean, the type's one metric.
// maxlen: the longest list of the handle
void launch_ivf_scan_u8(const IvfU8Scan &a, int64_t maxlen, hipStream_t s);
// Whether that scan stages its rows (exact integer sums, any summation order gives the same bits) or walks them one lane per
// row in the chain arithmetic: D % 16 == 0 (chain j is then byte j of every 4-byte word), rows and queries 16-byte aligned
static inline bool ivf_scan_u8_staged(int D, const void *X, const void *Q)
{
    return D % 16 == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Q)) & 15) == 0;
}
// The largest D at which no pair's total exceeds 2^24 (258 * 65025 < 2^24): the staged scans' totals form up to here, their
// chains form beyond
constexpr int IVF_U8_TOTALS_D = 258;

// The list-major form of the staged scan (kernels_ivf_u8_group.hip), for a batch whose queries share lists: the pairs are
// grouped as for the float32 tile (launch_ivf_group, lb_ivf.h) and a workgroup scores 128-row tiles of an item's list against
// its group of at most 64 queries (chains form: one 32-query column of it) on the i8 matrix cores, over the bytes shifted by
// 128 as they are staged.  The same keys in the same places, bit for bit.  Requires ivf_scan_u8_staged(a.b.D, a.X, a.Q) and
// a.b.L.nlist <= IVF_MAX_NLIST.  Seven launches: the grouping's six, the tile
hipError_t launch_ivf_scan_u8_tile(const IvfU8Scan &a, const IvfGroups &g, int64_t maxlen, hipStream_t s);

} // namespace lb
