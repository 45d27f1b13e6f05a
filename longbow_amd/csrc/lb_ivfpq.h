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

// workgroups per pair (query, probed list) of the residual scan: IPQ_GRID over the launch's pairs, no more than the tiles of the
// handle's longest list, at least one
inline int64_t ivfpq_rscan_groups(int64_t pairs, int64_t maxlen)
{
    const int64_t tiles = (maxlen + IPQ_TILE - 1) / IPQ_TILE;
    const int64_t per_pair = (IPQ_GRID + pairs - 1) / (pairs > 0 ? pairs : 1);
    const int64_t g = per_pair < tiles ? per_pair : tiles;
    return g < 1 ? 1 : g;
}

// The shape of a residual scan launch over `pairs` pairs of nq queries, pmax the most positions a query has, maxlen the longest
// list.  Strided: grid (pairs, groups), a pair's workgroups stride over its list; chosen while the longest list is at most two
// steps of that stride.  Beyond that one pair's serial tail is what the launch waits for, and the scan runs from a work list
// instead: an item is a pair and a run of `run` consecutive tiles of its list, the items of all pairs are numbered by a prefix
// sum over the pairs' tile counts (one small launch before the scan), and the scan has a workgroup per item.  `grid` is the host's
// bound of the items (the positions of all pairs are at most nq * pmax, and every pair adds at most one partial tile and one
// partial run); a workgroup beyond the device's count returns at once.
constexpr int IPQ_RUN_MAX = 8; // tiles per item at most: a table copy (M * 1024 B) per 8 tiles' rows at most
struct IvfpqRscanPlan {
    bool items;     // the work list, not the strided grid
    int64_t groups; // strided: workgroups per pair
    int run;        // work list: tiles per item
    int64_t grid;   // work list: workgroups launched
};
inline IvfpqRscanPlan ivfpq_rscan_plan(int64_t pairs, int64_t nq, int64_t pmax, int64_t maxlen)
{
    const int64_t groups = ivfpq_rscan_groups(pairs, maxlen), tiles_max = (maxlen + IPQ_TILE - 1) / IPQ_TILE;
    if (tiles_max <= 2 * groups) return IvfpqRscanPlan{false, groups, 0, 0};
    const int64_t tiles = pairs + (nq * pmax + IPQ_TILE - 1) / IPQ_TILE; // a bound of the tiles of all pairs
    int64_t run = (tiles + IPQ_GRID - 1) / IPQ_GRID;
    run = run < 1 ? 1 : run > IPQ_RUN_MAX ? IPQ_RUN_MAX : run;
    return IvfpqRscanPlan{true, 0, (int)run, pairs + (tiles + run - 1) / run};
}

// How a residual search fits its tables (M * 1024 bytes a pair) into `budget` bytes: `nb` queries a batch at most, each with all
// its np slots in one round, so that nb * np tables fit; only when one query's np tables do not fit, nb = 1 and the slots go in
// rounds of `slots` (the last one shorter).
struct IvfpqTablePlan {
    int64_t nb;    // queries per batch at most
    int64_t slots; // slots of a query per round: np, or fewer when nb == 1
};
inline IvfpqTablePlan ivfpq_table_plan(int64_t np, int M, int64_t budget)
{
    const int64_t fit = budget / ((int64_t)M * 1024) > 0 ? budget / ((int64_t)M * 1024) : 1; // tables the budget holds
    if (np <= fit) return IvfpqTablePlan{fit / (np > 0 ? np : 1), np};
    return IvfpqTablePlan{1, fit};
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

// ---- residual codes: res(v, l)[i] = v[i] - C[l][i], one f32 subtraction a component; C is [nlist][dims] ------------------------
// out[r] = res(X[r], assign[r]) for r in [0, cnt); a row whose list is outside [0, nlist) is not written
void launch_ivfpq_residual_rows(const float *X, const uint32_t *assign, const float *C, int64_t cnt, int dims, int nlist, float *out,
                                hipStream_t s);
// The pairs of a launch are slots [s0, s0 + ns) of every query of the batch: pair = q * ns + (slot - s0), a.nq * ns of them.
// rq[pair] = res(a.Q[q], a.probes[q][slot]), or zeros where that probe is no list of the handle (C: the handle's centroids)
void launch_ivfpq_residual_queries(const IvfBatch &a, int s0, int ns, const float *C, float *rq, hipStream_t s);
// keys[q][seg[q][slot] + i] = pack_entry(ADC distance under tables[pair], row) of the i-th position of the slot's list, for the
// pairs above: tables is [a.nq * ns][M][256] f32; lcodes, n as launch_ivfpq_scan; maxlen the longest list of a.L; item_off is
// scratch of a.nq * ns + 1 words for the work list (ivfpq_rscan_plan decides: one launch, or two with the list's prefix sum)
void launch_ivfpq_rscan(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n, int64_t maxlen,
                        uint32_t *item_off, hipStream_t s);
// the same under a row filter: a.L, rows and nvis as launch_ivfpq_scan_visible
void launch_ivfpq_rscan_visible(const IvfBatch &a, int s0, int ns, const float *tables, int M, const uint8_t *lcodes, int64_t n, int64_t maxlen,
                                uint32_t *item_off, const uint32_t *rows, int64_t nvis, hipStream_t s);

} // namespace lb
