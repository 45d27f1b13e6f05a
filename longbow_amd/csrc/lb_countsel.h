// lb_countsel.h -- exact top-k by counting: the method, and the pieces of it that kernels_bq.hip and kernels_sq8.hip share.
//
// A distance is a small integer and ties are the normal case (a corpus of identical codes is legal), so a search keeps no
// candidate list.  Per query:
//   hist    histogram of the distances (BQ: all 64*W + 1 values at once; SQ8: one 11/11/10-bit digit of S per pass, three
//           passes): LDS per workgroup, flushed with one atomic per non-empty bin
//   thresh  t = the smallest d with count(<= d) >= k, need = k - count(< t); fewer than k rows in all: t = 0x7fffffff (every
//           row is below it), need = 0                                                          [countsel_find]
//   count   rows below t and rows at t per (query, workgroup), workgroups owning contiguous runs of whole 256-row tiles, so
//           that positions order across workgroups                                              [countsel_plan]
//   scan    exclusive scan of those counts over the workgroups of a query                       [countsel_scan_kernel]
//   emit    rows below t, and the `need` lowest-positioned rows at t, to their slot among the query's k keys
//           (d << 32 | row): the tie rule is "the lowest positions win"                         [countsel_slot]
//   finish  sort the <= k keys of a query in LDS, write distances and labels, pad with FLT_MAX / -1
//                                                                                                [countsel_finish_kernel]
// Under a row filter the rows above are the positions of the ascending list of visible rows (launch_countsel_finish's posmap): positions order
// as rows do, so everything up to the emit runs over them unchanged, and the finish alone writes posmap[position] as the label.
// Workgroups meet at launch boundaries only; nothing is written past slot k - 1 and every count is bounded by the data's size,
// whatever the data.  Where the distance comes from (BQ recomputes it from LDS tiles in hist, count and emit; SQ8 reads its
// matrix S) stays with each index, and so do the hist, count and emit kernels around these pieces.
#pragma once
#include "lb_device.h"
#include "lb_select.h"

#include <type_traits>

namespace lb {

constexpr int COUNTSEL_ROWS = 256;          // rows of a tile, threads of a workgroup that walks tiles
constexpr uint32_t COUNTSEL_NO_SLOT = ~0u;  // countsel_slot: the row is not among the k

inline int64_t grid_cap(int64_t units, int64_t cap) { return units < 1 ? 1 : units < cap ? units : cap; }

// The query tile of a launch: the smallest of 1, 4, 8, 16 that holds nq (a single query pays for one), stepped down while
// fits(qt) refuses it (the launch's LDS budget).
template <class Fits> int pick_qt(int nq, Fits &&fits)
{
    int qt = nq <= 1 ? 1 : nq <= 4 ? 4 : nq <= 8 ? 8 : 16;
    while (qt > 1 && !fits(qt)) qt = qt == 16 ? 8 : qt == 8 ? 4 : 1;
    return qt;
}
template <class F> void with_qt(int qt, F &&f)
{
    switch (qt) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
    }
}

// The bin at which the running count of a histogram reaches `want`, and the rank still wanted inside it: serial, for one
// thread.  h: the bins; part[256]: the sums of 256 segments of `per` bins each (bins past the histogram's end count nothing).
// False when the whole histogram holds fewer than `want`.
__device__ __forceinline__ bool countsel_find(const uint32_t *h, const uint32_t *part, int per, uint32_t want, uint32_t &bin, uint32_t &need)
{
    uint32_t cum = 0;
    for (int seg = 0; seg < 256; seg++) {
        if (cum + part[seg] >= want) {
            for (int b = seg * per;; b++) { // ends inside the segment: its bins sum to part[seg]
                if (cum + h[b] >= want) {
                    bin = (uint32_t)b;
                    need = want - cum;
                    return true;
                }
                cum += h[b];
            }
        }
        cum += part[seg];
    }
    return false;
}

// The slot of this lane's row among its query's k keys, or COUNTSEL_NO_SLOT.  lt / eq: the row is below / at the threshold;
// blt / beq: their ballots over the wave; run[2]: slots the workgroup has used so far (below t, at t); wcnt[4][2]: this
// tile's counts per wave; lower: the mask of the lanes below this one; below: the query's rows below t in all.  The caller
// has made run and wcnt visible (a barrier) and updates run after every wave has read it.
__device__ __forceinline__ uint32_t countsel_slot(bool lt, bool eq, unsigned long long blt, unsigned long long beq, const uint32_t *run,
                                                  const uint32_t *wcnt, int wave, unsigned long long lower, uint32_t below, uint32_t need,
                                                  int k)
{
    uint32_t olt = run[0], oeq = run[1];
    for (int w = 0; w < wave; w++) {
        olt += wcnt[2 * w];
        oeq += wcnt[2 * w + 1];
    }
    olt += (uint32_t)__popcll(blt & lower);
    oeq += (uint32_t)__popcll(beq & lower);
    // rows at t: only the `need` lowest positions (oeq is the row's rank among them); nothing lands past slot k - 1
    const uint32_t slot = lt ? olt : below + oeq;
    return (lt || (eq && oeq < need)) && slot < (uint32_t)k ? slot : COUNTSEL_NO_SLOT;
}

} // namespace lb
