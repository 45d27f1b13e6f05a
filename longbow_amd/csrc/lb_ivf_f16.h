// lb_ivf_f16.h -- what ivf.hip (host) and kernels_ivf_f16.hip (device) share for an IVF-Flat handle whose rows are float16
// (lb_gpu_ivf_new_f16): the argument block of the list scan and its launcher.  The plan of a batch, the probes and the selection
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

} // namespace lb
