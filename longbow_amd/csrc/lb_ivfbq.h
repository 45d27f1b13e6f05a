// lb_ivfbq.h -- what ivfbq.hip (host) and kernels_ivfbq.hip (device) of the IVF-BQ index share: the argument block of the list
// scan and its two launchers.  The semantics are stated in include/longbow_gpu.h (lb_gpu_ivfbq_*).  The plan of a batch and the
// probes are the IVF-Flat index's (lb_ivf.h): IvfBatch is taken as it is, and the scan's own fields lie beside it here, so that
// the argument blocks of the kernels in kernels_ivf.hip, kernels_ivfpq.hip and kernels_ivfsq8.hip stay byte for byte what they
// were.  The list-major copy is launch_ivfpq_permute (lb_ivfpq.h) over rows of 8 * W bytes, the selection launch_ivfsq8_select
// (lb_ivfsq8.h): its keys (S << 32) | row and its emit float32(S) are what a Hamming distance needs.
#pragma once
#include "lb_ivf.h"

namespace lb {

constexpr int IBQ_ROWS = 256; // rows per tile of the scan == threads per workgroup

// One batch of queries as the list scan takes it (by value).  b.X, b.Q and b.qna are not read.
struct IvfBqScan {
    IvfBatch b;             // L, nq, probes, np, seg, keys, pmax
    const uint64_t *lcodes; // [n][W] the codes in list order: lcodes[pos] = codes[rows[pos]]
    const uint32_t *rows;   // [n] the rows of the lists of all n rows, which lcodes follows (without a filter: b.L.rows)
    int64_t n;              // rows stored: a list entry at or beyond it is read as n - 1 (never with the handle's own lists)
    int W;                  // u64 words of a row
    const uint64_t *qcodes; // [nq][W] the queries' codes, pad bits zero
    int64_t nvis;           // under a filter: entries the visible lists hold in all (voff[nlist]); else unused
};

// keys[q][seg[q][p] + i] = ((uint64_t)h << 32) | row of the i-th row of the p-th probed list, whose codes are the contiguous
// run lcodes[off[l], off[l + 1]); maxlen: the longest list of the handle
void launch_ivfbq_scan(const IvfBqScan &a, int64_t maxlen, hipStream_t s);
// the same under a row filter: b.L is the visible lists, whose entries are positions into `rows`: the i-th visible entry of
// list l is pos = vlist[voff[l] + i], its row rows[pos], its code lcodes[pos]; maxlen: the longest visible list
void launch_ivfbq_scan_visible(const IvfBqScan &a, int64_t maxlen, hipStream_t s);

} // namespace lb
