// kernels_ivfbq.hip -- the IVF-BQ index (ivfbq.hip; semantics in include/longbow_gpu.h, lb_gpu_ivfbq_*): the scan of the probed
// lists over sign-bit codes, without and under a row filter.  The plan of a batch, the lists and the visible lists are
// kernels_ivf.hip's, the codec kernels_bq.hip's, the list-major copy kernels_ivfpq.hip's, the selection kernels_ivfsq8.hip's.
//
// The codes lie list-major (lcodes[pos] = codes[rows[pos]]), so a probed list is one contiguous run of len * W words.  The scan is
// the list scans' walk (lb_list_scan.h) over the tile of kernels_bq.hip, restated here: a list per (query, probe slot), a
// tile is 256 rows, one lane owns a row.  A chunk is CW words of each of the tile's rows, fetched as coalesced 8-byte words
// (consecutive lanes read consecutive words of the run) into an LDS tile whose row stride is CW + 2 words: CW / 2 + 1 slots of
// 16 bytes, an odd number, so the rows are 16-byte aligned and the 16 lanes one ds_read_b128 cycle serves fall on 16 distinct
// slots.  Each lane reads its own row's CW words from it as CW / 2 such reads.  (At bq_tile's stride of CW + 1 words the rows
// are 8-byte aligned and the compiler pairs a lane's consecutive 8-byte reads into ds_read2_b64, half the bytes a cycle: by
// counter 17 % more LDS cycles for the same scan)  The stores are ds_write_b64 of consecutive words with a gap of
// two at every row boundary: a group of 16 lanes that holds a boundary wraps onto its own first banks, one extra array cycle
// inside the store's own transfer time.  The query's W words lie in LDS and are read wave-uniform
// (broadcast).  W <= 16 is one chunk (CW = 4, 8, 12 or 16); wider rows walk chunks of 8 words.  Words past W are zero on both
// sides.  h = sum of popcount(x ^ q) over the words, at most 8192, and every scanned row leaves one key (h << 32) | row: the u64
// order of the keys is the (h, row) order and kEntryMax padding sorts last.  Integer only.
//
// Under a row filter the list is the visible list, whose entries are positions into the lists of all rows: the code of an entry
// is lcodes[pos], still inside the probed list's run, and its row is rows[pos].  The gathers are then runs of CW (at most W)
// consecutive words per position.
#include "lb_device.h"
#include "lb_ivfbq.h"
#include "lb_list_scan.h"

#include <algorithm>
#include <type_traits>

namespace lb {

namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

} // namespace

// Work = (query, probe slot, 256-row tile of that list), found as lb_list_scan.h states and walked as it states, in this
// kernel's own text (below); of the work this scan takes the list's place in L.rows (off), not its rows.  A stage is 256 rows x CW words, with a register-held prefetch of the next
// one; the query's whole code lies behind the stage, zero past its last word.
// LDS: tile u64[IBQ_ROWS][CW + 2] | query u64[nchunks * CW]
template <int CW, bool VIS>
__global__ __launch_bounds__(IBQ_ROWS) void ivfbq_scan_kernel(IvfBqScan a)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t ibq_smem[];
    constexpr int LD = CW + 2; // an odd number of 16-byte slots
    uint64_t *lrow = ibq_smem;
    uint64_t *lq = lrow + IBQ_ROWS * LD;
    ListWork w;
    if (!ivf_list_work(a.b, IBQ_ROWS, w)) return;
    const int tid = threadIdx.x;
    const int W = a.W, nchunks = (W + CW - 1) / CW;
    const uint32_t ntiles = (w.len + IBQ_ROWS - 1) / IBQ_ROWS;
    const uint64_t *q_src = a.qcodes + (int64_t)w.q * W;
    const uint64_t last = (uint64_t)(a.n - 1);
    for (int idx = tid; idx < nchunks * CW; idx += IBQ_ROWS) lq[idx] = idx < W ? q_src[idx] : 0ull;

    // the position, in the lists of all rows, of entry e < len of this list: at most n - 1, whatever the lists hold
    auto entry_pos = [&](uint32_t e) -> uint64_t {
        uint64_t pos = (uint64_t)w.off + e;
        if (VIS) pos = pos < (uint64_t)a.nvis ? (uint64_t)a.b.L.rows[pos] : last;
        return pos < last ? pos : last;
    };

    // a thread's CW staging slots of a stage: word ch % CW of row ch / CW of the tile, ch = tid + 256 i
    uint64_t stg[CW];
    uint32_t rpos[CW]; // the positions behind them, of the tile being loaded (below 2^31)
    auto load_stage = [&](uint32_t tile, int c) {
        const uint32_t trow0 = tile * IBQ_ROWS;
#pragma unroll
        for (int i = 0; i < CW; i++) {
            const int ch = tid + IBQ_ROWS * i;
            const int r = ch / CW, wv = ch - r * CW;
            if (c == 0) {
                uint32_t e = trow0 + (uint32_t)r;
                if (e >= w.len) e = w.len - 1;
                rpos[i] = (uint32_t)entry_pos(e);
            }
            const int wd = c * CW + wv;
            // (a plain load: other queries of the batch probe the same list and find it in L2 / MALL)
            stg[i] = wd < W ? a.lcodes[(uint64_t)rpos[i] * (uint64_t)W + wd] : 0ull;
        }
    };
    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < CW; i++) {
            const int ch = tid + IBQ_ROWS * i;
            const int r = ch / CW, wv = ch - r * CW;
            lrow[r * LD + wv] = stg[i];
        }
    };

    uint32_t h = 0u; // the distance of this lane's row so far
    // a finished tile's key is written right after the next stage's loads are issued
    uint32_t pend_h = 0u, pend_tile = 0u;
    bool pending = false;
    auto flush = [&]() {
        const uint32_t e = pend_tile * IBQ_ROWS + tid;
        if (e < w.len) w.out[e] = ((uint64_t)pend_h << 32) | (uint64_t)a.rows[entry_pos(e)];
        pending = false;
    };

    // walk_list_tiles' walk (lb_list_scan.h) in this kernel's own text, kept in step with it by hand.  Built over the shared
    // walk the eight instantiations came out the same length with 37 - 64 instructions different (same registers and
    // occupancy), and three of 32 scan-slot rows missed the rule of LABNOTES R34.1, each by 0.2 % or 0.3 us: <8, plain> at
    // 1024 queries x 32 probes, <12, visible> at 1 x 8, <16, visible> at 1024 x 8.
    uint32_t tile = blockIdx.x;
    int c = 0;
    load_stage(tile, 0);
    write_stage();
    __syncthreads(); // (the query's code too)
    while (true) {
        uint32_t ntile = tile;
        int nc = c + 1;
        if (nc == nchunks) {
            nc = 0;
            ntile = tile + gridDim.x;
        }
        const bool has_next = ntile < ntiles;
        if (has_next) load_stage(ntile, nc);
        if (pending) flush();
        if (c == 0) h = 0u;
        {
            const u64x2 *xr = reinterpret_cast<const u64x2 *>(lrow + tid * LD); // (16-byte aligned: LD is even)
            const u64x2 *qc = reinterpret_cast<const u64x2 *>(lq + c * CW);
            int sum = 0;
#pragma unroll
            for (int g = 0; g < CW / 2; g++) {
                const u64x2 x = xr[g], q = qc[g];
                sum += __popcll(x.x ^ q.x) + __popcll(x.y ^ q.y);
            }
            h += (uint32_t)sum;
        }
        __syncthreads(); // every wave is done reading the stage
        if (has_next) write_stage();
        if (c == nchunks - 1) {
            pend_h = h;
            pend_tile = tile;
            pending = true;
        }
        __syncthreads();
        if (!has_next) break;
        tile = ntile;
        c = nc;
    }
    if (pending) flush();
}

namespace {

// the chunk rule of kernels_bq.hip (bq_cw)
int ibq_cw(int W) { return W <= 4 ? 4 : W <= 8 ? 8 : W <= 12 ? 12 : W <= 16 ? 16 : 8; }

template <bool VIS> void launch_ivfbq_scan_v(const IvfBqScan &a, int64_t maxlen, hipStream_t s)
{
    const int64_t pairs = (int64_t)a.b.nq * a.b.np;
    if (pairs <= 0 || maxlen <= 0 || a.n <= 0 || a.W <= 0) return;
    const dim3 grid = ivf_scan_grid(pairs, maxlen, IBQ_ROWS);
    const int cw = ibq_cw(a.W);
    const size_t lds = ((size_t)IBQ_ROWS * (cw + 2) + (size_t)((a.W + cw - 1) / cw) * cw) * 8; // at most 36,992 B (W = 16)
    auto go = [&](auto c) { hipLaunchKernelGGL((ivfbq_scan_kernel<decltype(c)::value, VIS>), grid, dim3(IBQ_ROWS), lds, s, a); };
    switch (cw) {
    case 4: go(std::integral_constant<int, 4>{}); break;
    case 8: go(std::integral_constant<int, 8>{}); break;
    case 12: go(std::integral_constant<int, 12>{}); break;
    default: go(std::integral_constant<int, 16>{}); break;
    }
}

} // namespace

void launch_ivfbq_scan(const IvfBqScan &a, int64_t maxlen, hipStream_t s) { launch_ivfbq_scan_v<false>(a, maxlen, s); }

void launch_ivfbq_scan_visible(const IvfBqScan &a, int64_t maxlen, hipStream_t s)
{
    if (a.nvis <= 0) return; // (every seg is 0: no key is read)
    launch_ivfbq_scan_v<true>(a, maxlen, s);
}

} // namespace lb
