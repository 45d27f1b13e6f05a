// lb_refine.h -- what refine.hip (host) and kernels_refine.hip (device) of lb_gpu_index_refine share: the argument block of the
// kernels and their launchers.  The semantics are stated in include/longbow_gpu.h (lb_gpu_index_refine).
#pragma once
#include "lb_device.h"

namespace lb {

// One batch of queries with c candidate rows each, as the refine kernels take it (by value).
struct RefineBatch {
    const void *X;       // [ntotal][D] rows: f32, or fp16 on a float16 index
    int D;
    int64_t ntotal;      // rows of the index, <= 2^32 - 1
    const float *Q;      // [nq][D]
    const float *qna;    // [nq] ||q||^2 in the call's order (cosine; else unused)
    int nq;
    const int64_t *rows; // [nq][c] the caller's shortlists: any values, any order
    int c;
    uint32_t *list;      // [nq][c]: list[q][0 .. len[q]) = the distinct entries of rows[q] inside [0, ntotal) (and live), ascending
    uint32_t *len;       // [nq]
    uint64_t *keys;      // [nq][c]: keys[q][i] = pack_entry(distance, list[q][i]) for i < len[q]
    const uint8_t *live; // nullable: [ntotal], a row with a zero byte has been removed and counts as outside the index
};

// list and len of every query from rows
void launch_refine_prepare(const RefineBatch &a, hipStream_t s);
// keys of every query from list and len; f16: the rows are fp16, widened exactly
void launch_refine_scan(int metric, int order, bool f16, const RefineBatch &a, hipStream_t s);

} // namespace lb
