// index_remove.hip -- lb_gpu_index_remove*, _nlive, _ndeleted and _compact (include/longbow_gpu.h): rows leave the flat index.
//
// Removal is a second per-row state beside the caller's filter: d_live (lb_index.h), which no filter call writes.  d_mask is
// the effective mask, filter AND live, so row_view and every search driver read what they always read; a removal clears the
// row's byte in both arrays and rebuilds the row list.  Compaction gives the space back: the survivors are gathered to the
// front in their order, in place, and the index is then what an index filled with the survivors alone would be.
// The bodies run inside guard() (lb_handle.h) under the exclusive lock, on add_stream.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_host.h"
#include "lb_index.h"
#include "lb_remove.h"

#include <algorithm>
#include <vector>

using namespace lb;

namespace {

// After the kernel that cleared the bytes: the count, the handle's state and the row list.  d_cnt: the launch's counter.
int64_t commit_removed(lb_gpu_index *h, const uint32_t *d_cnt)
{
    hipStream_t s = h->add_stream;
    uint32_t removed = 0;
    LB_LAUNCH_CHECK();
    LB_HIP(hipMemcpyAsync(&removed, d_cnt, sizeof removed, hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    if (removed == 0) return 0;
    h->n_dead += removed;
    h->has_mask = true;
    try {
        rebuild_rowmap(h);
    } catch (const HipErr &) { // (as finish_add: searches fall back to the per-row mask test)
        (void)hipGetLastError();
        h->rowmap_on = false;
        h->n_visible = h->n;
    }
    return removed;
}

// d_live and d_mask as the kernels will clear them (lb_remove.h: `ready`): without a mask in force d_mask holds a cleared filter's
// bytes, so "every row" is written first
RemovalArrays arrays_for_removal(lb_gpu_index *h)
{
    if (!h->has_mask && h->n > 0) LB_HIP(hipMemsetAsync(h->d_mask.get(), 1, (size_t)h->n, h->add_stream));
    return RemovalArrays{h->d_live.get(), h->d_mask.get()};
}

// n positions (host or device memory) -> *n_removed; the caller holds the exclusive lock
int remove_positions(lb_gpu_index *h, int64_t n, const int64_t *rows, bool on_device, int64_t *n_removed)
{
    Lease buf; // [counter, 16 bytes | the positions when they come from the host]
    return guard(h, h->add_stream, [&]() -> int {
        int64_t removed = 0;
        if (h->n > 0) {
            LB_HIP(hipSetDevice(h->device));
            removed = remove_by_position(h->device, h->add_stream, buf, n, rows, on_device, h->n, [&] { return arrays_for_removal(h); },
                                         [&](const uint32_t *d_cnt) { return commit_removed(h, d_cnt); });
        }
        if (n_removed) *n_removed = removed;
        return LB_OK;
    });
}

// n labels of the host; the caller holds the exclusive lock
int remove_labels(lb_gpu_index *h, int64_t n, const int64_t *labels, int64_t *n_removed)
{
    if (!h->has_ids) return remove_positions(h, n, labels, false, n_removed); // the labels of such an index are its positions
    Lease buf; // [counter, 16 bytes | the set]
    return guard(h, h->add_stream, [&]() -> int {
        int64_t removed = 0;
        if (h->n > 0) {
            LB_HIP(hipSetDevice(h->device));
            removed = remove_by_id(h->device, h->add_stream, buf, n, labels, h->d_ids.get(), h->n, [&] { return arrays_for_removal(h); },
                                   [&](const uint32_t *d_cnt) { return commit_removed(h, d_cnt); });
        }
        if (n_removed) *n_removed = removed;
        return LB_OK;
    });
}

} // namespace

extern "C" {

int lb_gpu_index_remove(lb_gpu_index *h, int64_t n, const int64_t *labels, int64_t *n_removed)
{
    if (!h || n < 0 || (n > 0 && !labels)) return LB_ERR_INVALID_ARG;
    if (n == 0) { if (n_removed) *n_removed = 0; return LB_OK; }
    std::unique_lock<std::shared_mutex> g(h->mu);
    return remove_labels(h, n, labels, n_removed);
}

int lb_gpu_index_remove_device(lb_gpu_index *h, int64_t n, const int64_t *d_labels, int64_t *n_removed)
{
    if (!h || n < 0 || (n > 0 && !d_labels)) return LB_ERR_INVALID_ARG;
    if (n == 0) { if (n_removed) *n_removed = 0; return LB_OK; }
    std::unique_lock<std::shared_mutex> g(h->mu);
    if (!h->has_ids) return remove_positions(h, n, d_labels, true, n_removed);
    // ids: the set is sorted on the host (n is small beside ntotal, and this is on no search's path)
    std::vector<int64_t> host;
    const int rc = guard(h, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        host.resize((size_t)n);
        LB_HIP(hipMemcpy(host.data(), d_labels, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
        return LB_OK;
    });
    return rc != LB_OK ? rc : remove_labels(h, n, host.data(), n_removed);
}

int lb_gpu_index_remove_rows(lb_gpu_index *h, int64_t n, const int64_t *rows, int64_t *n_removed)
{
    if (!h || n < 0 || (n > 0 && !rows)) return LB_ERR_INVALID_ARG;
    if (n == 0) { if (n_removed) *n_removed = 0; return LB_OK; }
    std::unique_lock<std::shared_mutex> g(h->mu);
    return remove_positions(h, n, rows, false, n_removed);
}

int64_t lb_gpu_index_nlive(const lb_gpu_index *h)
{
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_index *>(h)->mu);
    return h->n - h->n_dead;
}

int64_t lb_gpu_index_ndeleted(const lb_gpu_index *h)
{
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_index *>(h)->mu);
    return h->n_dead;
}

int lb_gpu_index_compact(lb_gpu_index *h, int64_t *old_rows, int64_t cap)
{
    if (!h) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    const int64_t n_old = h->n, nlive = h->n - h->n_dead;
    if (old_rows && cap < nlive) {
        h->set_error("old_rows has room for %lld rows, the index holds %lld live ones", (long long)cap, (long long)nlive);
        return LB_ERR_INVALID_ARG;
    }
    if (h->n_dead == 0) { // nothing to do: every row stays where it is
        if (old_rows)
            for (int64_t j = 0; j < nlive; j++) old_rows[j] = j;
        return LB_OK;
    }
    Lease lmap, lscr, lgather; // the survivor list, launch_compact_mask's scratch (its last word: the first removed row), a round's rows
    return guard(h, h->add_stream, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        hipStream_t s = h->add_stream;
        const size_t row_bytes = (size_t)h->dim * h->elem_bytes();
        // what moves with a row: its elements, its id, its filter byte (the norms are recomputed below, to the same bits)
        const size_t idb = h->has_ids ? sizeof(int64_t) : 0, mb = h->has_filter ? 1 : 0;
        const int64_t R = std::min<int64_t>(compact_round_rows(row_bytes + idb + mb), std::max<int64_t>(nlive, 1));
        // every buffer before the first launch: a refusal leaves the index as it was
        char *gx = nullptr, *gi = nullptr, *gm = nullptr;
        lease_layout(lgather, h->device, [&](Carve cv) {
            gx = cv.take<char>((size_t)R * row_bytes);
            gi = cv.take<char>((size_t)R * idb);
            gm = cv.take<char>((size_t)R * mb);
            return cv.off;
        });
        std::vector<uint32_t> hmap(old_rows ? (size_t)nlive : 0);
        // 1. the ascending survivor list, map[j] >= j, and the first removed row: the rows before it stay where they are
        int64_t first = 0;
        if (const int rc = compact_survivors(h, h->device, h->d_live.get(), n_old, nlive, lmap, lscr, hmap, &first, s)) return rc;
        // 2. the rounds of R destination rows (lb_remove.h: compact_walk)
        const CompactArray arrays[3] = {{h->d_X, row_bytes, gx}, {h->d_ids.get(), idb, gi}, {h->d_mask.get(), mb, gm}};
        compact_walk(arrays, 3, lmap.as<uint32_t>(), first, nlive, R, h->device, s);
        // the norms of the rows where they now lie, and with them the statistics over the rows that are left (launch_row_norms
        // gives a row the bits it gave it at Add: one wave per row, whatever the row's position)
        const uint32_t norm_init[2] = {0u, 0x7f800000u};
        uint32_t nbits[2] = {0, 0};
        LB_HIP(hipMemcpyAsync(h->d_maxnorm2.get(), norm_init, sizeof norm_init, hipMemcpyHostToDevice, s));
        if (h->i8_rows)
            launch_row_norms_i8(h->rows_i8(), nlive, h->dim, h->norm2_i8(), s);
        else
            with_rows(h, [&](auto Xr) { launch_row_norms(Xr, nlive, h->dim, h->d_norm2.get(), h->d_rnorm.get(), h->d_maxnorm2.get(), s); });
        LB_HIP(hipMemcpyAsync(nbits, h->d_maxnorm2.get(), sizeof nbits, hipMemcpyDeviceToHost, s));
        if (nlive > 0) LB_HIP(hipMemsetAsync(h->d_live.get(), 0xff, (size_t)nlive, s));
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        // 3. the rows are where they belong: committed, and nothing below may fail the call
        h->n = nlive;
        h->n_dead = 0;
        h->has_mask = h->has_filter; // (the filter's bytes came along; without one there is no mask any more)
        set_norm_flags(h, nbits);
        for (int64_t j = 0; j < (int64_t)hmap.size(); j++) old_rows[j] = (int64_t)hmap[(size_t)j];
        // 4. what was derived from the rows that are gone is derived again, as finish_add ends
        drop_split_image(h);
        drop_f16_image(h);
        h->xh_declined_n = 0;
        h->xh_shed = false;
        h->f16_skip.store(0);
        h->f16_span.store(16);
        h->kc_hint.store(0);
        h->kc_hint_left.store(0);
        try {
            sync_split_image(h);
        } catch (const HipErr &) {
            (void)hipGetLastError();
            h->cand_mode.store(LB_CAND_AUTO);
            drop_split_image(h);
        }
        sync_f16_image(h);
        try {
            rebuild_rowmap(h);
        } catch (const HipErr &) {
            (void)hipGetLastError();
            h->rowmap_on = false;
            h->n_visible = h->n;
        }
        return LB_OK;
    });
}

#ifdef LB_DIAG
// rows per round of the compaction's gather at most (0: the scratch bound alone): small corpora then walk many rounds
void lb_debug_set_compact_round_rows(long long rows) { g_compact_round_rows.store(rows); }
#endif

} // extern "C"
