// lb_ivfsq8.h -- what ivfsq8.hip (host) and kernels_ivfsq8.hip (device) of the IVF-SQ8 index share: the argument block of the
// list scan and the launchers.  The semantics are stated in include/longbow_gpu.h (lb_gpu_ivfsq8_*).  The plan of a batch and
// the probes are the IVF-Flat index's (lb_ivf.h): IvfBatch is taken as it is, and the scan's own fields lie beside it here, so
// that the argument blocks of the kernels in kernels_ivf.hip and kernels_ivfpq.hip stay byte for byte what they were.
#pragma once
#include "lb_ivf.h"

namespace lb {

constexpr int ISQ_ROWS = 128; // rows per tile of the scan == threads per workgroup

// One batch of queries as the list scan takes it (by value).  b.X, b.Q and b.qna are not read.
struct IvfSq8Scan {
    IvfBatch b;            // L, nq, probes, np, seg, keys, pmax
    const uint8_t *codes;  // [n][stride] rows in insertion order, pad bytes zero, 16-byte aligned
    int64_t n;             // rows stored: a list entry at or beyond it is read as row n - 1 (never with the handle's own lists)
    int stride;            // bytes of a row: a multiple of 16
    const uint8_t *qcodes; // [nq][stride] the queries' codes, pad bytes zero, 16-byte aligned
    const int32_t *qnorms; // [nq] sum of squares of each query's code
};

// keys[q][seg[q][p] + i] = ((uint64_t)S << 32) | row of the i-th row of the p-th probed list; maxlen: the longest list of the handle
void launch_ivfsq8_scan(const IvfSq8Scan &a, int64_t maxlen, hipStream_t s);
// launch_ivf_select over such keys: the k smallest of each query, ascending as integers -> dist = float32(S) / labels [nq][k]
// (ids nullable: the row itself), padded FLT_MAX / -1
void launch_ivfsq8_select(const IvfBatch &a, int k, const int64_t *ids, float *dist, int64_t *labels, hipStream_t s);

} // namespace lb
