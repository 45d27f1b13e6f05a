// lb_ivfpq4.h -- what ivfpq4.hip (host) and kernels_ivfpq4.hip (device) of the IVF-PQ4 index share beyond lb_ivfpq.h and lb_pq4.h:
// the table budget rule at 64 bytes a subspace and the launchers of the ADC scans over the packed 4-bit codes of a query's
// probed lists.  The semantics are stated in include/longbow_gpu.h (lb_gpu_ivfpq4_*).
//
// The tile (IPQ_TILE), the grid rule (ivfpq_scan_groups, ivfpq_rscan_groups) and the residual scan's plan (ivfpq_rscan_plan, its
// run of up to IPQ_RUN_MAX tiles an item included) are the IVF-PQ handle's.  IPQ_GRID = 512 was reasoned from one 96 KB table a
// CU; here a workgroup holds M * 64 bytes of LDS and it is its 1024 threads that bound a CU to two workgroups (2048 thread
// slots), so 512 workgroups are the chip's 256 CUs filled exactly once: a larger grid adds table copies and no residency.
#pragma once
#include "lb_ivfpq.h"
#include "lb_pq4.h"

namespace lb {

// ivfpq_table_plan over tables of M * 16 f32: `nb` queries a batch at most with all np slots of each in one round, or, when one
// query's np tables do not fit `budget` bytes, one query a batch and rounds of `slots` slots
inline IvfpqTablePlan ivfpq4_table_plan(int64_t np, int M, int64_t budget)
{
    const int64_t bytes = (int64_t)M * PQ4_K * 4;
    const int64_t fit = budget / bytes > 0 ? budget / bytes : 1; // tables the budget holds
    if (np <= fit) return IvfpqTablePlan{fit / (np > 0 ? np : 1), np};
    return IvfpqTablePlan{1, fit};
}

// keys[q][t] = pack_entry(ADC distance, row) of the t-th position of the concatenation of q's probed lists, t in [0, seg[q][np]):
// tables is [a.nq][M][16] f32, lcodes the list-major packed codes of a.L (pq4_row_bytes(M) bytes a row), n the rows they hold
void launch_ivfpq4_scan(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, hipStream_t s);
// the same under a row filter: a.L is the visible lists, which hold positions into `rows`, the rows of the lists of all n rows that
// lcodes follows; nvis is what they hold in all
void launch_ivfpq4_scan_visible(const IvfBatch &a, const float *tables, int M, const uint8_t *lcodes, int64_t n, const uint32_t *rows,
                                int64_t nvis, hipStream_t s);
// The residual scan over the pairs of launch_ivfpq_residual_queries (slots [s0, s0 + ns) of every query of the batch):
// keys[q][seg[q][slot] + i] = pack_entry(ADC distance under tables[pair], row) of the i-th position of the slot's list; tables is
// [a.nq * ns][M][16] f32; maxlen the longest list of a.L; item_off is scratch of a.nq * ns + 1 words for the work list
// (ivfpq_rscan_plan decides: one launch, or two with the list's prefix sum)
void launch_ivfpq4_rscan(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n, int64_t maxlen,
                         uint32_t *item_off, hipStream_t s);
// the same under a row filter: a.L, rows and nvis as launch_ivfpq4_scan_visible
void launch_ivfpq4_rscan_visible(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n,
                                 int64_t maxlen, uint32_t *item_off, const uint32_t *rows, int64_t nvis, hipStream_t s);

} // namespace lb
