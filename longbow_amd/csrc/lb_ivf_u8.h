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

} // namespace lb
