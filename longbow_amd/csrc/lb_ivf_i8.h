// lb_ivf_i8.h -- what ivf.hip (host) and kernels_ivf_i8.hip (device) share for an IVF-Flat handle whose rows are int8
// (lb_gpu_ivf_new_i8): the argument block of the list scan and its launcher.  The plan of a batch, the probes and the selection
// are the f32 handle's (lb_ivf.h): IvfBatch is taken as it is, and the scan's own fields lie beside it here, as in lb_ivf_f16.h.
#pragma once
#include "lb_ivf.h"

namespace lb {

// One batch of queries as the int8 list scan takes it (by value).  b.X and b.Q are not read: b.Q is the batch's queries widened
// to f32, which the coarse index probes with; the scan reads the int8 queries themselves.
struct IvfI8Scan {
    IvfBatch b;      // D, L, nq, probes, np, seg, keys, pmax
    const int8_t *X; // [n][D] rows in insertion order
    const int8_t *Q; // [nq][D] the batch's queries
};

// launch_ivf_scan over int8 rows and int8 queries: keys[q][seg[q][p] + i] = entry of the i-th row of the p-th probed list, the
// distance being the flat int8 index's (kernels_i8.hip; lb_i8_exact.h), bit for bit.  metric: METRIC_L2 or METRIC_DOT.
// maxlen: the longest list of the handle
void launch_ivf_scan_i8(int metric, const IvfI8Scan &a, int64_t maxlen, hipStream_t s);

} // namespace lb
