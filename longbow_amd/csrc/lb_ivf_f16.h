// lb_ivf_f16.h -- what ivf.hip (host) and kernels_ivf_f16.hip / kernels_ivf_f16_group.hip (device) share for an IVF-Flat handle
// whose rows are float16 (lb_gpu_ivf_new_f16): the argument block of the list scan and its launchers.  The plan of a batch, the probes and the selection
// are the f32 handle's (lb_ivf.h): IvfBatch is taken as it is, and the scan's own field lies beside it here, so that the argument
// blocks of the kernels in kernels_ivf.hip stay byte for byte what they were.
#pragma once
#include "lb_ivf.h"

namespace lb {

// One batch of queries as the fp16 list scan takes it (by value).  b.X is not read.
struct IvfF16Scan {
    IvfBatch b;        // D, L, Q, qna, nq, probes, np, seg, keys, pmax
    const _Float16 *X; // [n][D] rows in insertion order, IEEE binary16
};

// launch_ivf_scan over fp16 rows: keys[q][seg[q][p] + i] = entry of the i-th row of the p-th probed list, every element widened
// to f32 and summed in the chains of lb_exact.h, so the keys are those of launch_ivf_scan over the widened rows, bit for bit.
// maxlen: the longest list of the handle
void launch_ivf_scan_f16(int metric, int order, const IvfF16Scan &a, int64_t maxlen, hipStream_t s);
// Whether that scan stages its rows through LDS in 16-byte pieces of eight halves or walks them one lane per row: D % 8 == 0,
// rows and queries 16-byte aligned
static inline bool ivf_scan_f16_staged(int D, const void *X, const void *Q)
{
    return D % 8 == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Q)) & 15) == 0;
}

// The list-major form of the staged scan (kernels_ivf_f16_group.hip), for a batch whose queries share lists: the pairs are
// grouped as for the float32 tile (launch_ivf_group, lb_ivf.h) and a workgroup scores 64-row tiles of an item's list against its
// group of at most 64 queries, the rows fp16 in LDS and widened as they are read.  The same chains, so the same keys in the same
// places, bit for bit.  Requires ivf_scan_f16_staged(a.b.D, a.X, a.b.Q) and a.b.L.nlist <= IVF_MAX_NLIST.  Seven launches: the
// grouping's six, the tile
hipError_t launch_ivf_scan_f16_tile(int metric, int order, const IvfF16Scan &a, const IvfGroups &g, int64_t maxlen, hipStream_t s);

} // namespace lb
