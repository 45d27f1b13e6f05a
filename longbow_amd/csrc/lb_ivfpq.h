// lb_ivfpq.h -- what ivfpq.hip (host) and kernels_ivfpq.hip (device) of the IVF-PQ index share beyond lb_ivf.h: the launchers of
// the list-major copy of the codes and of the ADC scan over a query's probed lists, without and under a row filter.  The
// semantics are stated in include/longbow_gpu.h (lb_gpu_ivfpq_*).
#pragma once
#include "lb_ivf.h"

namespace lb {

constexpr int IPQ_TILE = 1024; // positions per tile of the scan == threads per workgroup
constexpr int IPQ_GRID = 512;  // workgroups a scan launch aims at: the chip's 256 CUs twice over (one workgroup a CU holds its table)

// workgroups per query of the scan: enough tiles for the longest query, no more than IPQ_GRID over the batch
inline int64_t ivfpq_scan_groups(int nq, int64_t pmax)
{
    const int64_t tiles = (pmax + IPQ_TILE - 1) / IPQ_TILE;
    const int64_t per_query = (IPQ_GRID + nq - 1) / (nq > 0 ? nq : 1);
    return tiles < 1 ? 1 : tiles < per_query ? tiles : per_query;
}

// lcodes[pos] = codes[L.rows[pos]] for pos in [0, n): the codes in list order, M bytes a row
void launch_ivfpq_permute(const uint8_t *codes, const uint32_t *rows, int64_t n, int M, uint8_t *lcodes, hipStream_t s);

// keys[q][t] = pack_entry(ADC distance, row) of the t-th position of the concatenation of q's probed lists, t in [0, seg[q][np]):
// a.X, a.Q and a.qna are not read; tables is [a.nq][M][256] f32, lcodes the list-major codes of a.L, n the rows they hold
void launch_ivfpq_scan(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, hipStream_t s);
// the same under a row filter: a.L is the visible lists, which hold positions into `rows`, the rows of the lists of all n rows that
// lcodes follows; nvis is what they hold in all (voff[nlist]).  t runs over the concatenation of q's probed visible lists
void launch_ivfpq_scan_visible(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, const uint32_t *rows, int64_t nvis,
                               hipStream_t s);

} // namespace lb
