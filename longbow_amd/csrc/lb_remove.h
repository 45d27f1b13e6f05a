// lb_remove.h -- what the handles that can forget rows share on the host: the flat index (index_remove.hip) and the IVF handles
// (lb_ivf_host.h).  The kernels are kernels_remove.hip's and kernels_filter.hip's (lb_device.h).  Header-only, nothing exported.
//
//   * removal_set: the labels of a removal by id as launch_remove_ids takes them; remove_by_position / remove_by_id: what a
//     removal enqueues between the handle's own preparation and its own commit;
//   * compact_survivors: the ascending list of the live rows and the first removed one, checked against the host's count;
//   * compact_walk: the in-place gather of every per-row array through a bounded scratch, in rounds.  The bound
//     (kCompactScratch), the rows of a round (compact_round_rows) and the diagnostic library's hook on them
//     (lb_debug_set_compact_round_rows, index_remove.hip) are defined here, once.
#pragma once
#include "lb_device.h"
#include "lb_handle.h"

#include <algorithm>
#include <atomic>
#include <vector>

namespace lb {
#pragma GCC visibility push(hidden)

// bytes of gather scratch a round of a compaction may lease; a round's rows follow from it (compact_round_rows)
constexpr size_t kCompactScratch = (size_t)256 << 20;
inline std::atomic<long long> g_compact_round_rows{0}; // test hook: rows per round at most (0: what the scratch bound gives)

// rows per round when a row and what moves with it take per_row bytes of the scratch
inline int64_t compact_round_rows(size_t per_row)
{
    int64_t r = std::max<int64_t>(1, (int64_t)(kCompactScratch / per_row));
    const long long forced = g_compact_round_rows.load();
    if (forced > 0) r = std::min<int64_t>(r, forced);
    return r;
}

// The set of a removal by id: ascending and distinct, without -1 (the padding of a result list names no row)
inline std::vector<int64_t> removal_set(const int64_t *labels, int64_t n)
{
    std::vector<int64_t> set(labels, labels + n);
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    const auto pad = std::lower_bound(set.begin(), set.end(), (int64_t)-1);
    if (pad != set.end() && *pad == -1) set.erase(pad);
    return set;
}

// What a removal enqueues on s, inside the caller's guard.  buf: the caller's lease, declared outside that guard: [counter, 16 bytes |
// the values that come from the host].  ready() leaves the handle's live bytes and its effective mask as the kernel will clear
// them and returns the two; commit(d_cnt) drains s, reads the launch's counter and commits -> the rows newly removed.
struct RemovalArrays {
    uint8_t *live, *mask;
};

// n positions, in host or device memory, of a handle of ntotal rows
template <class Ready, class Commit>
int64_t remove_by_position(int device, hipStream_t s, Lease &buf, int64_t n, const int64_t *rows, bool on_device, int64_t ntotal, Ready &&ready,
                           Commit &&commit)
{
    buf.reset(device, 16 + (on_device ? 0 : (size_t)n * sizeof(int64_t)));
    uint32_t *d_cnt = buf.as<uint32_t>();
    const int64_t *d_rows = rows;
    LB_HIP(hipMemsetAsync(d_cnt, 0, 16, s));
    if (!on_device) {
        int64_t *up = reinterpret_cast<int64_t *>(buf.as<char>() + 16);
        LB_HIP(hipMemcpyAsync(up, rows, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        d_rows = up;
    }
    const RemovalArrays a = ready();
    launch_remove_rows(d_rows, n, ntotal, a.live, a.mask, d_cnt, s);
    return commit(d_cnt);
}

// n labels of the host on a handle whose ntotal rows carry the ids d_ids: every live row under one of them goes
template <class Ready, class Commit>
int64_t remove_by_id(int device, hipStream_t s, Lease &buf, int64_t n, const int64_t *labels, const int64_t *d_ids, int64_t ntotal, Ready &&ready,
                     Commit &&commit)
{
    const std::vector<int64_t> set = removal_set(labels, n);
    if (set.empty()) return 0;
    buf.reset(device, 16 + set.size() * sizeof(int64_t));
    uint32_t *d_cnt = buf.as<uint32_t>();
    int64_t *d_set = reinterpret_cast<int64_t *>(buf.as<char>() + 16);
    LB_HIP(hipMemsetAsync(d_cnt, 0, 16, s));
    LB_HIP(hipMemcpyAsync(d_set, set.data(), set.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    const RemovalArrays a = ready();
    launch_remove_ids(d_ids, ntotal, d_set, (int64_t)set.size(), a.live, a.mask, d_cnt, s);
    return commit(d_cnt); // (drains the stream: `set` may go)
}

// The ascending survivor list of live[0, n_old) into lmap (map[j] >= j), read back into hmap[0, hmap.size()) when the caller sized
// it, and *first = the first removed row: the rows before it stay where they are.  lmap and lscr are leased here (room for every
// row: the count is checked after the fact); the caller declares them outside its guard.  Drains s.  A count that differs from
// the host's nlive is LB_ERR_INTERNAL with a last_error text, and nothing has been written but the two leases.
inline int compact_survivors(HandleCore *h, int device, const uint8_t *live, int64_t n_old, int64_t nlive, Lease &lmap, Lease &lscr,
                             std::vector<uint32_t> &hmap, int64_t *first, hipStream_t s)
{
    const int64_t words = compact_scratch_words(n_old);
    lmap.reset(device, (size_t)n_old * sizeof(uint32_t));
    lscr.reset(device, (size_t)(words + 1) * sizeof(uint32_t)); // (its last word: the first removed row)
    uint32_t *map = lmap.as<uint32_t>(), *scr = lscr.as<uint32_t>();
    launch_compact_mask(live, n_old, map, scr, s);
    LB_HIP(hipMemsetAsync(scr + words, 0xff, sizeof(uint32_t), s));
    launch_first_dead(live, n_old, scr + words, s);
    uint32_t tail[2] = {0, 0}; // survivors counted, first removed row
    LB_HIP(hipMemcpyAsync(tail, scr + (words - 1), sizeof tail, hipMemcpyDeviceToHost, s));
    if (!hmap.empty()) LB_HIP(hipMemcpyAsync(hmap.data(), map, hmap.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LB_LAUNCH_CHECK();
    LB_HIP(hipStreamSynchronize(s));
    if ((int64_t)tail[0] != nlive || (int64_t)tail[1] >= n_old) {
        h->set_error("compact: %u rows live on the device, %lld on the host", tail[0], (long long)nlive);
        return LB_ERR_INTERNAL;
    }
    *first = (int64_t)tail[1];
    return LB_OK;
}

// A per-row array that a compaction moves: rows of `bytes` bytes at `base`, and the round's scratch for them (room for the round's
// rows; it overlaps nothing).  bytes == 0: the handle has no such array and nothing moves.
struct CompactArray {
    void *base;
    size_t bytes;
    void *scratch;
};

// Rounds of R destination rows over [first, nlive): a launch gathers map[r0, r0 + cnt) of every array into its scratch, a copy puts
// the scratch at [r0, r0 + cnt).  No launch reads what it writes, and the sources of every later round lie at or beyond r0 + cnt
// (map[j] >= j), which the copies before them on the stream have not touched.  Enqueues on s and does not drain it.
inline void compact_walk(const CompactArray *arrays, int narrays, const uint32_t *map, int64_t first, int64_t nlive, int64_t R, int device,
                         hipStream_t s)
{
    for (int64_t r0 = first; r0 < nlive; r0 += R) {
        const int64_t cnt = std::min(R, nlive - r0);
        for (int i = 0; i < narrays; i++)
            if (arrays[i].bytes) launch_gather_rows(arrays[i].base, map + r0, cnt, arrays[i].bytes, arrays[i].scratch, device, s);
        for (int i = 0; i < narrays; i++) {
            const CompactArray &a = arrays[i];
            if (a.bytes)
                LB_HIP(hipMemcpyAsync(static_cast<char *>(a.base) + (size_t)r0 * a.bytes, a.scratch, (size_t)cnt * a.bytes, hipMemcpyDeviceToDevice, s));
        }
    }
}

#pragma GCC visibility pop
} // namespace lb
