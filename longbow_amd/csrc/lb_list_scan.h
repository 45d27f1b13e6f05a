// lb_list_scan.h -- what the list scans share (kernels_ivf.hip, kernels_ivf_f16.hip, kernels_ivf_i8.hip, kernels_ivfsq8.hip,
// kernels_ivfbq.hip, kernels_refine.hip): a unit of work is a list of rows, one lane owns one row, and a workgroup walks the
// tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its list, every tile staged through LDS a chunk at a time.  Here, each once:
// which list a workgroup of an IVF scan works on, how many workgroups a launch places along a list, and the walk itself.  What a
// stage holds and the arithmetic over it are the kernels' own.
#pragma once
#include "lb_ivf.h"

#include <algorithm>
#include <type_traits>

namespace lb {

// What a workgroup of an IVF list scan works on: pair = (query, probe slot), wave-uniform.
struct ListWork {
    int q;
    uint32_t off;         // the list's first entry in L.rows
    uint32_t len;         // entries of the list
    const uint32_t *rmap; // L.rows + off: the list's rows, ascending
    uint64_t *out;        // the list's keys of this query
};

constexpr unsigned IVF_PAIRS_Y = 32768; // (query, probe) pairs along grid dimension y; the rest along z (both < 65536)

// false: nothing to do.  tile_rows: rows per tile of the calling kernel.
__device__ __forceinline__ bool ivf_list_work(const IvfBatch &a, int tile_rows, ListWork &w)
{
    const int64_t pair = (int64_t)blockIdx.y + (int64_t)blockIdx.z * gridDim.y;
    if (pair >= (int64_t)a.nq * a.np) return false;
    w.q = (int)(pair / a.np);
    const int p = (int)(pair % a.np);
    const int64_t l = a.probes[pair];
    if (l < 0 || l >= a.L.nlist) return false;
    w.off = a.L.off[l];
    w.len = a.L.off[l + 1] - w.off;
    if ((uint64_t)blockIdx.x * (uint32_t)tile_rows >= w.len) return false; // (an empty list among them)
    const uint32_t seg = a.seg[(int64_t)w.q * (a.np + 1) + p];
    if ((int64_t)seg + w.len > a.pmax) return false; // never with distinct probes: the keys of a query stay inside its pmax
    w.rmap = a.L.rows + w.off;
    w.out = a.keys + (int64_t)w.q * a.pmax + seg;
    return true;
}

// Workgroups along one list of `tiles` tiles, with `items` lists to scan: enough workgroups to fill the chip (256 CUs, 4
// workgroups each) four times over and no more; a workgroup walks the rest of its list's tiles itself.
static inline int64_t list_scan_gx(int64_t items, int64_t tiles)
{
    return std::min<int64_t>(tiles, std::max<int64_t>(1, (4096 + items - 1) / items));
}

// The grid of an IVF list scan: tiles of the handle's longest list along x, the (query, probe) pairs along y and z.
static inline dim3 ivf_scan_grid(int64_t pairs, int64_t maxlen, int tile_rows)
{
    const int64_t tiles = (maxlen + tile_rows - 1) / tile_rows;
    const unsigned gy = (unsigned)std::min<int64_t>(pairs, IVF_PAIRS_Y);
    const unsigned gz = (unsigned)((pairs + gy - 1) / gy); // <= 1024 queries x 65536 lists / 32768 = 2048
    return dim3((unsigned)list_scan_gx(pairs, tiles), gy, gz);
}

// f(metric, order) with the runtime metric and order as std::integral_constant: the scans that are templates over both
template <class F> static inline void with_metric_order(int metric, int order, F &&f)
{
    auto with_order = [&](auto m) {
        if (order == ORDER_UNROLL4) f(m, std::integral_constant<int, ORDER_UNROLL4>{});
        else f(m, std::integral_constant<int, ORDER_SEQ>{});
    };
    if (metric == METRIC_L2) with_order(std::integral_constant<int, METRIC_L2>{});
    else if (metric == METRIC_COS) with_order(std::integral_constant<int, METRIC_COS>{});
    else with_order(std::integral_constant<int, METRIC_DOT>{});
}

// The walk of a workgroup over its list's tiles: the (tile, chunk) sequence is one flat pipeline over one LDS stage plus a
// register-held prefetch of the next one, wrapping from a tile's last chunk to the next tile's first.
//   load_stage(tile, c)  global -> registers, chunk c of the tile (c == 0: the tile's row numbers too)
//   write_stage()        registers -> LDS
//   consume(c)           the lane's row over the stage in LDS; c == 0 starts the row's accumulators
//   finish()             after a tile's last chunk: the accumulators become the value flush will write
//   flush(tile)          writes that tile's keys: one stage late, right after the next stage's loads are issued
// has_next is fixed before the loads; the last tile's keys are written behind the loop.
// ivf_scan_f16_kernel and ivf_scan_i8_kernel are built over it.  ivf_scan_kernel, ivfsq8_scan_kernel, ivfbq_scan_kernel and
// refine_scan_kernel restate it in their own text for the measurements named at their loops (Debt): a fix to the
// walk is made there too.
template <class Load, class Write, class Consume, class Finish, class Flush>
__device__ __forceinline__ void walk_list_tiles(uint32_t ntiles, int nchunks, Load &&load_stage, Write &&write_stage, Consume &&consume,
                                                Finish &&finish, Flush &&flush)
{
    uint32_t tile = blockIdx.x, pend_tile = 0;
    int c = 0;
    bool pending = false;
    load_stage(tile, 0);
    write_stage();
    __syncthreads(); // (whatever else the kernel put into LDS before the walk too)
    while (true) {
        uint32_t ntile = tile;
        int nc = c + 1;
        if (nc == nchunks) {
            nc = 0;
            ntile = tile + gridDim.x;
        }
        const bool has_next = ntile < ntiles;
        if (has_next) load_stage(ntile, nc);
        if (pending) {
            flush(pend_tile);
            pending = false;
        }
        consume(c);
        __syncthreads(); // every wave is done reading the stage
        if (has_next) write_stage();
        if (c == nchunks - 1) {
            finish();
            pend_tile = tile;
            pending = true;
        }
        __syncthreads();
        if (!has_next) break;
        tile = ntile;
        c = nc;
    }
    if (pending) flush(pend_tile);
}

} // namespace lb
