// lb_ivf_host.h -- the host side that the IVF handles share: what ivf.hip (lb_gpu_ivf, rows), ivfpq.hip (lb_gpu_ivfpq, PQ codes),
// ivfsq8.hip (lb_gpu_ivfsq8, SQ8 codes) and ivfbq.hip (lb_gpu_ivfbq, BQ codes) have in common beyond lb_handle.h.  Header-only,
// host-only, nothing exported.
//
// The contract:
//   * IvfPartition is the coarse partition of a handle's rows: the inner exact f32 index over the centroids, the list of each row
//     and the inverted lists over them.  It is the member `part` of IvfHandle, which every handle derives from and which also
//     holds what the row filter (lb_handle.h) adds to a partition: the visible lists.  The functions here take
//     (CodeHandle *h, IvfPartition &P, ...) or an IvfHandle *p, the entry-point templates a T *p with p->part and p->timing;
//   * the rules at the head of lb_handle.h hold: every pooled Lease that a function here enqueues work on is the caller's, declared
//     outside its guard(); coarse_fail drains the stream before leases go back; searches and reads take `mu` shared, adds and
//     reserve take it alone.  Everything that takes a stream runs inside the caller's guard() and throws as its body does;
//   * growth is all or nothing and is written once: ivf_grow, over the row arrays a handle names (IvfRowArray), in the order
//     stated there.  A handle's *_grow is that call and nothing else;
//   * the add is written once: ivf_add.  It writes behind the stored rows and into the pair of lists that is not in use, and
//     commits last, in the order stated there, with nothing that throws after the first committed field.  Under a filter the new
//     rows are visible and the visible lists of all rows are built and committed with the rest (ivf_add_visible,
//     ivf_commit_visible); on a handle that has removed rows they are live (ivf_add_live).  A handle gives it its
//     grow, the piece size, where a piece's f32 rows come from, what it stores from them and what it derives from the new lists;
//     a lease of the handle's own is declared by the handle, ahead of the call and so outside ivf_add's guard();
//   * the filter calls rebuild the visible lists through ivf_visible_builder, the `built` hook of filter_set / filter_column;
//   * rows can be removed (ivf_remove_*, ivf_compact; entry points on lb_gpu_ivf, lb_gpu_ivfpq and lb_gpu_ivfsq8; lb_gpu_ivfbq has
//     none yet and never holds a removed row).  IvfHandle::live is a second per-row state beside the caller's filter, allocated
//     at the first removal, which no filter call writes.  From then on filter.mask is the EFFECTIVE mask, the caller's filter AND
//     live, and filter.on says that an effective mask is in force, a caller's filter or removed rows or both (has_filter tells
//     which); lists() and sizes() read what they always read.  A removal clears the rows' bytes in both arrays and rebuilds the
//     row list and the visible lists as a filter call does; the filter calls AND `live` into the mask they write (filter.live,
//     lb_handle.h); an add makes its rows live; IvfGrowth carries the bytes.  Compaction gathers the survivors to the front in
//     place (lb_remove.h) and derives the lists from the stored assignments, which move with the rows: nothing is assigned
//     again, and on the code handles nothing is encoded again, the codes being the rows that move.  A handle with `positions`
//     keeps a list-major copy of its codes beside the lists: a removal leaves that copy alone (the visible lists it builds hold
//     positions into the copy of ALL rows), and compaction writes the copy of the pair not in use from the compacted codes and
//     the new lists through ivf_compact's `relist` hook;
//   * ivf_search is the one search loop.  A call travels as a record (IvfCall), a handle's fixed choices as another
//     (IvfSearchForm); the handle supplies its scratch pieces and the launches between the plan and the selection, which are told
//     about the lists the batch walks through IvfWalk; ctx is polled before every launch, a cancelled search publishes no stats,
//     and the events of a profiled search fall where the handle's timing slots say.  A row bitmap given with the call is the
//     entry-point templates' business (call_filter) and, in the loop, IvfCallWalk's; a plain search is that search without one.
#pragma once
#include "lb_handle.h"
#include "lb_ivf.h"
#include "lb_remove.h"

#include <atomic>
#include <functional>
#include <initializer_list>
#include <stdexcept>
#include <vector>

namespace lb {
#pragma GCC visibility push(hidden) // the instantiations over the handles' types stay out of the library's exports

constexpr int64_t kQueryBatch = 1024;              // queries per batch at most
constexpr int64_t kKeyScratch = (int64_t)1 << 30;  // bytes of keys a batch may hold
// bytes of ADC tables a batch of a residual IVF-PQ search may hold (a table per probed list of each query): one pooled lease,
// at M = 96 room for 10,922 tables
constexpr int64_t kTableScratch = (int64_t)1 << 30;
constexpr int kMaxTimingSlots = 5;

struct IvfPartition {
    int nlist = 0;
    lb_gpu_index *coarse = nullptr; // the centroids: same device, dims and order as the handle
    std::vector<float> h_cent;      // [nlist][dims]
    DevBuf<int64_t> d_ids;          // [capacity] when ids were given
    bool has_ids = false;
    DevBuf<uint32_t> d_assign;      // [capacity]: list of each row
    // the lists are built for all rows by every add, into the pair that is not in use: a failed add leaves the old ones
    DevBuf<uint32_t> d_off[2];      // [nlist + 1]
    DevBuf<uint32_t> d_list[2];     // [capacity]
    int cur = 0;
    std::vector<int64_t> h_sizes;   // [nlist]: sizes grids and scratch without a device round trip
    int64_t stats[4] = {0, 0, 0, 0}; // of the last search (under err_mu)
    std::atomic<bool> profiling{false};
    ~IvfPartition() { lb_gpu_index_free(coarse); }
    IvfLists all_lists(int i) const { return IvfLists{d_off[i].get(), d_list[i].get(), nlist}; }
    int64_t hbm_bytes() const
    {
        return (int64_t)(d_ids.count() * 8 + (d_assign.count() + d_list[0].count() + d_list[1].count() + d_off[0].count() + d_off[1].count()) * 4) +
               lb_gpu_index_hbm_bytes(coarse);
    }
};

// What both IVF handles are: a partition and, for the row filter, the visible lists.  A search under a filter walks the visible
// lists: of each list the entries whose row's mask byte is non-zero, in the list's order.  An entry is the row itself (IVF-Flat)
// or, with `positions`, its position in the lists of all rows (IVF-PQ: the list-major codes are addressed by it, and the pair of
// all lists gives its row).  They are built by every filter call and by every add to a filtered handle, into the pair that is not
// in use; filter.n_visible is d_voff[vcur][nlist].  filter.rowmap is rebuilt by the filter calls only and nothing here reads it.
struct IvfHandle : FilteredHandle { // searches and reads share mu; adds, reserve and the filter calls take it alone
    IvfPartition part;              // the centroids and the lists of all rows
    bool positions = false;         // what a visible list holds; fixed at creation
    DevBuf<uint32_t> d_voff[2];     // [nlist + 1]
    DevBuf<uint32_t> d_vlist[2];    // [capacity] from the first filter on
    int vcur = 0;
    std::vector<int64_t> h_vsizes;  // [nlist]: what part.h_sizes is to the lists
    float build_ms = 0;             // of the last profiled build of the visible lists (under err_mu): its launches alone
    // removal: live[r] is zero for a removed row (whole words: launch_remove_rows); n_dead of the n rows are removed.  While
    // n_dead > 0 filter.live points here and filter.on holds.  has_filter (read while filter.on): a caller's filter is in force
    DevBuf<uint8_t> live;           // [capacity] from the first removal on
    int64_t n_dead = 0;
    bool has_filter = false;
    // what a search walks, and the sizes that go with it
    IvfLists lists() const { return filter.on ? IvfLists{d_voff[vcur].get(), d_vlist[vcur].get(), part.nlist} : part.all_lists(part.cur); }
    const std::vector<int64_t> &sizes() const { return filter.on ? h_vsizes : part.h_sizes; }
    int64_t visible_bytes() const // what the row filter holds on the device
    {
        return (int64_t)((d_voff[0].count() + d_voff[1].count() + d_vlist[0].count() + d_vlist[1].count()) * 4 + filter.mask.count() + live.count() +
                         (filter.rowmap.count() + filter.scratch.count()) * 4);
    }
};

// ---- opening ----------------------------------------------------------------------------------------------------------------
// A handle (T: an IvfHandle) of `dims` dimensions over `nlist` centroids, the caller having checked its arguments: the host fields
// and offsets of the partition and of the visible lists, init(p) for the handle's own, then the inner index of `metric` and `order`
// with the centroids in it.
template <class T, class Init>
T *ivf_open(int device, int dims, int metric, int order, int nlist, const float *centroids, int *out_status, Init &&init)
{
    int inner = LB_OK;
    T *h = handle_open<T>(device, out_status, [&](T *p) {
        IvfPartition &P = p->part;
        p->dims = dims;
        P.nlist = nlist;
        P.h_cent.assign(centroids, centroids + (size_t)nlist * dims);
        P.h_sizes.assign((size_t)nlist, 0);
        p->h_vsizes.assign((size_t)nlist, 0);
        for (DevBuf<uint32_t> *offs : {P.d_off, p->d_voff})
            for (int i = 0; i < 2; i++) {
                offs[i].alloc((size_t)nlist + 1);
                LB_HIP(hipMemset(offs[i].get(), 0, ((size_t)nlist + 1) * 4));
            }
        init(p);
        P.coarse = lb_gpu_index_new(device, dims, metric, &inner);
        if (!P.coarse) return;
        inner = lb_gpu_index_set_order(P.coarse, order);
        if (inner == LB_OK) inner = lb_gpu_index_add(P.coarse, nlist, centroids, nullptr);
        LB_HIP(hipSetDevice(device));
    });
    if (h && inner != LB_OK) { // the centroids did not get onto the device
        handle_free(h);
        if (out_status) *out_status = inner;
        return nullptr;
    }
    return h;
}

// ---- growth -----------------------------------------------------------------------------------------------------------------
// The capacity that room for `need` rows (and for ids, if wanted) asks for: the present one when only the ids are missing, -1 when
// nothing is.
inline int64_t ivf_grow_to(const CodeHandle *h, const IvfPartition &P, int64_t need, bool want_ids, size_t row_bytes)
{
    const bool ids_missing = want_ids && P.d_ids.count() < (size_t)std::max<int64_t>(h->capacity, 1);
    if (need <= h->capacity && !ids_missing) return -1;
    return need <= h->capacity ? h->capacity : grow_capacity(h->capacity, need, row_bytes);
}

// The share of the partition and of the visible lists in ivf_grow to `cap` rows: stage() allocates and fills and may throw,
// commit() moves and cannot.
constexpr size_t live_bytes(int64_t cap) { return ((size_t)cap + 3) & ~(size_t)3; } // (whole words: launch_remove_rows)

struct IvfGrowth {
    DevBuf<int64_t> ids;
    DevBuf<uint32_t> assign, list[2], vlist[2];
    DevBuf<uint8_t> live;
    bool want_ids = false, resize = false, filtered = false;
    void stage(const IvfHandle *h, int64_t cap, bool with_ids)
    {
        const IvfPartition &P = h->part;
        want_ids = with_ids;
        resize = cap != h->capacity;
        filtered = h->filter.on;
        if (want_ids) {
            ids.alloc((size_t)cap);
            if (h->n > 0 && P.has_ids) LB_HIP(hipMemcpy(ids.get(), P.d_ids.get(), (size_t)h->n * 8, hipMemcpyDeviceToDevice));
        }
        if (!resize) return;
        assign.alloc((size_t)cap);
        for (DevBuf<uint32_t> &l : list) l.alloc((size_t)cap);
        if (h->n > 0) { // (of the lists the pair in use alone)
            LB_HIP(hipMemcpy(assign.get(), P.d_assign.get(), (size_t)h->n * 4, hipMemcpyDeviceToDevice));
            LB_HIP(hipMemcpy(list[P.cur].get(), P.d_list[P.cur].get(), (size_t)h->n * 4, hipMemcpyDeviceToDevice));
        }
        if (h->live) { // a handle that has removed rows keeps their state
            live.alloc(live_bytes(cap));
            if (h->n > 0) LB_HIP(hipMemcpy(live.get(), h->live.get(), (size_t)h->n, hipMemcpyDeviceToDevice));
        }
        if (!filtered) return; // an active filter keeps its visible lists
        for (DevBuf<uint32_t> &v : vlist) v.alloc((size_t)cap);
        if (h->filter.n_visible > 0)
            LB_HIP(hipMemcpy(vlist[h->vcur].get(), h->d_vlist[h->vcur].get(), (size_t)h->filter.n_visible * 4, hipMemcpyDeviceToDevice));
    }
    void commit(IvfHandle *h) noexcept
    {
        IvfPartition &P = h->part;
        if (want_ids) P.d_ids = std::move(ids);
        if (!resize) return;
        P.d_assign = std::move(assign);
        for (int i = 0; i < 2; i++) P.d_list[i] = std::move(list[i]);
        if (live) {
            h->live = std::move(live);
            if (h->filter.live) h->filter.live = h->live.get();
        }
        if (filtered)
            for (int i = 0; i < 2; i++) h->d_vlist[i] = std::move(vlist[i]);
    }
};

// One of a handle's own row arrays (rows or codes, of any element type, kept as bytes): a single buffer, or the pair indexed by
// part.cur, which an add or a compaction writes whole into the half not in use.
struct IvfRowArray {
    DevBuf<uint8_t> *buf; // the buffer, or the first of the pair
    size_t row_bytes;
    bool pair;
};

// Room for `need` rows (and for ids, if wanted).  All or nothing: no old buffer is replaced before every new one is allocated and
// filled.  The capacity grows by the first array's row.
inline void ivf_grow(IvfHandle *p, int64_t need, bool want_ids, std::initializer_list<IvfRowArray> arrays)
{
    const int64_t cap = ivf_grow_to(p, p->part, need, want_ids, arrays.begin()->row_bytes); // 1. the capacity
    if (cap < 0) return;
    IvfGrowth g;
    std::vector<DevBuf<uint8_t>> fresh(2 * arrays.size());
    g.stage(p, cap, want_ids);                                                               // 2. the partition's share
    if (g.resize) {                                                                          // 3. the handle's own arrays
        size_t i = 0;
        for (const IvfRowArray &a : arrays)
            for (int j = 0; j < (a.pair ? 2 : 1); j++) fresh[i++].alloc((size_t)cap * a.row_bytes);
        i = 0;
        for (const IvfRowArray &a : arrays) { // (of a pair the half in use alone)
            const int j = a.pair ? p->part.cur : 0;
            if (p->n > 0) LB_HIP(hipMemcpy(fresh[i + j].get(), a.buf[j].get(), (size_t)p->n * a.row_bytes, hipMemcpyDeviceToDevice));
            i += a.pair ? 2 : 1;
        }
        p->filter.grow(p->n, cap);                                                           // 4. the last step that can fail
    }
    g.commit(p);                                                                             // 5. nothing below throws
    if (!g.resize) return;
    size_t i = 0;
    for (const IvfRowArray &a : arrays)
        for (int j = 0; j < (a.pair ? 2 : 1); j++) a.buf[j] = std::move(fresh[i++]);
    p->capacity = cap;
}

// ---- the steps of an add ----------------------------------------------------------------------------------------------------
inline int ivf_ids_consistent(CodeHandle *h, const IvfPartition &P, const int64_t *ids)
{
    if (h->n == 0 || (ids != nullptr) == P.has_ids) return LB_OK;
    h->set_error("ids are given on every add or on none: the handle's rows have %s", P.has_ids ? "ids" : "none");
    return LB_ERR_INVALID_ARG;
}

// the coarse index's own refusal becomes the handle's; what the call enqueued on s is drained before its pooled buffers go back
inline int coarse_fail(CodeHandle *h, const IvfPartition &P, int rc, hipStream_t s)
{
    (void)hipStreamSynchronize(s);
    if (rc == LB_ERR_CANCELLED || rc == LB_ERR_DEADLINE) return ctx_fail(h, rc);
    h->set_error("coarse quantiser: %s", lb_gpu_last_error(P.coarse));
    return rc;
}

// bytes of `lab` for ivf_assign of up to `rows` rows: their labels and distances
inline size_t ivf_assign_bytes(int64_t rows) { return up16((size_t)rows * 8) + (size_t)rows * 4; }

// The lists of the `cnt` device rows d_rows, to be stored as rows [row0, row0 + cnt): the k = 1 search of each over the centroids,
// narrowed into assign.  Enqueues on s and does not drain it, except to refuse.
inline int ivf_assign(CodeHandle *h, IvfPartition &P, int64_t row0, int64_t cnt, const float *d_rows, Lease &lab, hipStream_t s)
{
    int64_t *d_lab = lab.as<int64_t>();
    float *d_dist = reinterpret_cast<float *>(lab.as<char>() + up16((size_t)cnt * 8));
    if (const int rc = lb_gpu_index_search_device(P.coarse, cnt, d_rows, 1, d_dist, d_lab, s)) return coarse_fail(h, P, rc, s);
    launch_ivf_narrow(d_lab, cnt, P.d_assign.get() + row0, s);
    return LB_OK;
}

// The lists of rows [0, total) from assign, into the pair not in use, in two halves, so that a handle can enqueue what it derives
// from the new lists between them.  The launches:
inline void ivf_sort_lists(CodeHandle *h, IvfPartition &P, int64_t total, Lease &hist, hipStream_t s)
{
    const int nxt = 1 - P.cur;
    hist.reset(h->device, ivf_sort_hist_words(total, P.nlist) * 4);
    LB_HIP(launch_ivf_sort(P.d_assign.get(), total, P.nlist, hist.as<uint32_t>(), P.d_off[nxt].get(), P.d_list[nxt].get(), s));
}
// The read-back of the new lists' sizes: drains s.  The caller commits `sizes` and the pair.
inline int ivf_read_lists(CodeHandle *h, IvfPartition &P, int64_t total, std::vector<int64_t> &sizes, hipStream_t s)
{
    std::vector<uint32_t> h_off((size_t)P.nlist + 1);
    sizes.resize((size_t)P.nlist);
    LB_LAUNCH_CHECK();
    LB_HIP(hipMemcpyAsync(h_off.data(), P.d_off[1 - P.cur].get(), h_off.size() * 4, hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    if ((int64_t)h_off[P.nlist] != total) {
        h->set_error("the lists hold %lld of %lld rows", (long long)h_off[P.nlist], (long long)total);
        return LB_ERR_INTERNAL;
    }
    for (int l = 0; l < P.nlist; l++) sizes[l] = (int64_t)h_off[l + 1] - (int64_t)h_off[l];
    return LB_OK;
}

// ---- the visible lists ------------------------------------------------------------------------------------------------------
// The visible lists of mask[0, n) over the lists `L` of those n rows, into pair `to`; drains s.  Nothing of the handle but that
// pair's buffers is written: the caller commits vsizes, `to` and the count it gets back.  scratch: a lease declared outside the
// caller's guard.
inline int64_t ivf_build_visible(IvfHandle *p, const IvfLists &L, int64_t n, int to, Lease &scratch, std::vector<int64_t> &vsizes, hipStream_t s)
{
    const int nlist = p->part.nlist;
    std::vector<uint32_t> h_voff((size_t)nlist + 1);
    vsizes.resize((size_t)nlist);
    if (p->d_vlist[to].count() < (size_t)p->capacity) p->d_vlist[to].alloc((size_t)p->capacity);
    scratch.reset(p->device, ivf_visible_scratch_bytes(n));
    const bool prof = p->part.profiling.load();
    EventH ev[2];
    if (prof) {
        for (EventH &e : ev) LB_HIP(hipEventCreate(&e.h));
        LB_HIP(hipEventRecord(ev[0], s));
    }
    LB_HIP(launch_ivf_visible(p->filter.mask.get(), L, n, p->positions, scratch.p, p->d_voff[to].get(), p->d_vlist[to].get(), s));
    LB_LAUNCH_CHECK();
    if (prof) LB_HIP(hipEventRecord(ev[1], s));
    LB_HIP(hipMemcpyAsync(h_voff.data(), p->d_voff[to].get(), h_voff.size() * 4, hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    if (prof) {
        float ms = 0.f;
        LB_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        std::lock_guard<std::mutex> g(p->err_mu);
        p->build_ms = ms;
    }
    for (int l = 0; l < nlist; l++) vsizes[l] = (int64_t)h_voff[l + 1] - (int64_t)h_voff[l];
    return (int64_t)h_voff[nlist];
}

// what a filter call hands to the shell (lb_handle.h: `built`): the visible lists of the mask it has just written
// has_filter: what the handle's flag becomes when the build has succeeded
inline auto ivf_visible_builder(IvfHandle *p, Lease &scratch, bool has_filter)
{
    return [p, &scratch, has_filter](hipStream_t s) {
        std::vector<int64_t> vsizes;
        const int to = 1 - p->vcur;
        const int64_t nv = ivf_build_visible(p, p->part.all_lists(p->part.cur), p->n, to, scratch, vsizes, s);
        if (nv != p->filter.n_visible) throw std::logic_error("the visible lists do not hold the visible rows"); // (LB_ERR_INTERNAL)
        p->h_vsizes.swap(vsizes);
        p->vcur = to;
        p->has_filter = has_filter;
    };
}

// the filter calls of a handle: lb_handle.h's with the visible lists built behind the mask
inline int ivf_set_filter(IvfHandle *p, const uint8_t *mask, int64_t n)
{
    Lease vis;
    return filter_set(p, mask, n, ivf_visible_builder(p, vis, mask != nullptr));
}
template <class T> int ivf_filter_column(IvfHandle *p, const T *column, int64_t n, T value, int op, const uint8_t *validity, int64_t voff, int combine)
{
    Lease vis;
    return filter_column<T>(p, column, n, value, op, validity, voff, combine, ivf_visible_builder(p, vis, true));
}

// An add's step under a filter, after the lists of all `total` rows are in the partition's pair not in use: the new rows
// [p->n, total) are visible (their mask bytes belong to nobody until the commit), and the visible lists of all rows are built from
// the new lists into the pair not in use.  Drains s; -> the visible rows, for ivf_commit_visible
inline int64_t ivf_add_visible(IvfHandle *p, int64_t total, Lease &scratch, std::vector<int64_t> &vsizes, hipStream_t s)
{
    LB_HIP(hipMemsetAsync(p->filter.mask.get() + p->n, 1, (size_t)(total - p->n), s));
    return ivf_build_visible(p, p->part.all_lists(1 - p->part.cur), total, 1 - p->vcur, scratch, vsizes, s);
}
inline void ivf_commit_visible(IvfHandle *p, std::vector<int64_t> &vsizes, int64_t nvis) noexcept
{
    p->h_vsizes.swap(vsizes);
    p->vcur = 1 - p->vcur;
    p->filter.n_visible = nvis;
}

// ---- removal ----------------------------------------------------------------------------------------------------------------
// An add's step on a handle that holds live bytes: the new rows [p->n, total) are live (their bytes belong to nobody until the
// commit).  Enqueues on s, ahead of a step of the add that drains it.
inline void ivf_add_live(IvfHandle *p, int64_t total, hipStream_t s)
{
    if (p->live && total > p->n) LB_HIP(hipMemsetAsync(p->live.get() + p->n, 0xff, (size_t)(total - p->n), s));
}

// Removed rows are hidden by the effective mask alone.  A filter call or a removal that failed half way (lb_handle.h: "leaves the
// handle without a filter") must not show them again: a search refuses until a filter call has put the mask back.
inline int ivf_live_ok(IvfHandle *p)
{
    if (p->n_dead == 0 || p->filter.on) return LB_OK;
    p->set_error("a failed call left the handle's %lld removed rows without their mask: set_filter puts it back", (long long)p->n_dead);
    return LB_ERR_INTERNAL;
}

// ---- the add ----------------------------------------------------------------------------------------------------------------
// n rows (`vectors`: only looked at for being there), with ids or without, from host or device memory.  The handle gives:
//   grow(total, want_ids)        its *_grow
//   piece_cap                    rows assigned at a time at most
//   rows(r0, cnt, piece, s)      -> the device-resident f32 rows [r0, r0 + cnt) of the add, for ivf_assign: enqueued on s, valid until
//                                the piece's store has been enqueued.  The pieces come in order; at r0 == 0 it sizes whatever lease
//                                it fills for pieces of up to `piece` rows
//   store(d_rows, r0, cnt, piece, s)  enqueues what the handle keeps of them as rows [p->n + r0, ..) (codes; their lists are in
//                                part.d_assign by then); ivf_no_store for a handle whose rows() has stored them
//   relist(nxt, total, s)        what it derives from the new lists of all rows: ivf_compact's hook, called between the sort and
//                                the read-back of the sizes
// Leases that rows() and store() fill are the handle's, declared ahead of this call and so outside the guard() here.  Rows, codes
// and lists of the new rows are written behind the stored ones, where they belong to nobody until the commit; the lists of all
// rows go into the pair not in use.  Between pieces the stream is drained (a piece's leases are reused by the next); behind the
// last one ivf_read_lists drains it.
inline void ivf_no_store(const float *, int64_t, int64_t, int64_t, hipStream_t) {}
template <class Grow, class Rows, class Store, class Relist>
int ivf_add(IvfHandle *p, int64_t n, const void *vectors, const int64_t *ids, bool on_device, int64_t piece_cap, Grow &&grow, Rows &&rows,
            Store &&store, Relist &&relist)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    IvfPartition &P = p->part;
    if (const int st = ivf_ids_consistent(p, P, ids)) return st;
    if (const int st = rows_fit(p, p->n, n)) return st;
    Lease lab, hist, vis;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        const int64_t total = p->n + n;
        std::vector<int64_t> sizes, vsizes;
        const bool filtered = p->filter.on;
        grow(total, ids != nullptr);
        if (ids) LB_HIP(hipMemcpyAsync(P.d_ids.get() + p->n, ids, (size_t)n * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        // 1. the new rows, a piece at a time: their lists, and what the handle stores of them
        const int64_t piece = std::min(n, piece_cap);
        lab.reset(p->device, ivf_assign_bytes(piece));
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            const float *d_rows = rows(r0, cnt, piece, s);
            if (const int rc = ivf_assign(p, P, p->n + r0, cnt, d_rows, lab, s)) return rc;
            store(d_rows, r0, cnt, piece, s);
            if (r0 + piece < n) {
                LB_LAUNCH_CHECK();
                LB_HIP(hipStreamSynchronize(s));
            }
        }
        // 2. the lists of all rows, and what the handle derives from them, into the pair not in use
        const int nxt = 1 - P.cur;
        ivf_add_live(p, total, s); // (a handle that has removed rows: the new ones are live)
        ivf_sort_lists(p, P, total, hist, s);
        relist(nxt, total, s);
        if (const int rc = ivf_read_lists(p, P, total, sizes, s)) return rc;
        // 3. under a filter the new rows are visible: the visible lists of all rows, from the new lists, into the pair not in use
        //    (the mask bytes behind the stored rows belong to nobody until the commit)
        const int64_t nvis = filtered ? ivf_add_visible(p, total, vis, vsizes, s) : 0;
        // 4. commit, in this order; nothing below throws
        if (filtered) ivf_commit_visible(p, vsizes, nvis);
        P.h_sizes.swap(sizes);
        P.cur = nxt;
        P.has_ids = ids != nullptr;
        p->n = total;
        return LB_OK;
    });
}

// What a code handle's rows() is: the caller's device rows as they are, or its host rows staged a piece at a time.
struct IvfAddSource {
    const float *vectors;
    bool on_device;
    int device, dims;
    Lease vec; // (outside ivf_add's guard with the struct)
    const float *operator()(int64_t r0, int64_t cnt, int64_t piece, hipStream_t s)
    {
        const float *src = vectors + (size_t)r0 * dims;
        if (on_device) return src;
        if (r0 == 0) vec.reset(device, (size_t)piece * dims * 4);
        LB_HIP(hipMemcpyAsync(vec.p, src, (size_t)cnt * dims * 4, hipMemcpyHostToDevice, s));
        return vec.as<float>();
    }
};

// lb_remove.h's `ready`: the live bytes (allocated by the first removal), the mask as the kernel will clear it (without one in
// force, "every row" is written first) and every buffer of the rebuild behind the kernel, so that once bytes are cleared nothing
// but a device fault fails the call.  vis: the caller's lease for ivf_build_visible.
inline RemovalArrays ivf_removal_ready(IvfHandle *p, Lease &vis, hipStream_t s)
{
    RowFilter &f = p->filter;
    if (!p->live) {
        DevBuf<uint8_t> nl;
        nl.alloc(live_bytes(p->capacity));
        LB_HIP(hipMemsetAsync(nl.get(), 0xff, (size_t)p->n, s));
        p->live = std::move(nl);
    }
    if (!f.on) {
        f.reserve(p->n, p->capacity);
        LB_HIP(hipMemsetAsync(f.mask.get(), 1, (size_t)p->n, s));
    }
    const int to = 1 - p->vcur;
    if (p->d_vlist[to].count() < (size_t)p->capacity) p->d_vlist[to].alloc((size_t)p->capacity);
    vis.reset(p->device, ivf_visible_scratch_bytes(p->n));
    return RemovalArrays{p->live.get(), f.mask.get()};
}

// lb_remove.h's `commit`: the count; if rows went, the handle's state, then the row list and the visible lists as a filter call
// builds them, into the pair not in use.  A call that removes nothing commits nothing.
inline int64_t ivf_commit_removed(IvfHandle *p, const uint32_t *d_cnt, Lease &vis, hipStream_t s)
{
    uint32_t removed = 0;
    LB_LAUNCH_CHECK();
    LB_HIP(hipMemcpyAsync(&removed, d_cnt, sizeof removed, hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    if (removed == 0) return 0;
    RowFilter &f = p->filter;
    const bool had_filter = f.on && p->has_filter;
    p->n_dead += removed;
    f.live = p->live.get();
    f.on = false; // as filter_set: a failure from here on leaves the handle without its mask (ivf_live_ok)
    f.rebuild(p->n, s);
    ivf_visible_builder(p, vis, had_filter)(s);
    f.on = true;
    return removed;
}

// n positions (host or device memory) -> *n_removed; the caller holds the exclusive lock
inline int ivf_remove_positions(IvfHandle *p, int64_t n, const int64_t *rows, bool on_device, int64_t *n_removed)
{
    Lease buf, vis;
    return guard(p, p->stream, [&]() -> int {
        int64_t removed = 0;
        if (p->n > 0) {
            LB_HIP(hipSetDevice(p->device));
            hipStream_t s = p->stream;
            removed = remove_by_position(p->device, s, buf, n, rows, on_device, p->n, [&] { return ivf_removal_ready(p, vis, s); },
                                         [&](const uint32_t *d_cnt) { return ivf_commit_removed(p, d_cnt, vis, s); });
        }
        if (n_removed) *n_removed = removed;
        return LB_OK;
    });
}

// n labels of the host; the caller holds the exclusive lock
inline int ivf_remove_labels(IvfHandle *p, int64_t n, const int64_t *labels, int64_t *n_removed)
{
    if (!p->part.has_ids) return ivf_remove_positions(p, n, labels, false, n_removed); // the labels of such a handle are its positions
    Lease buf, vis;
    return guard(p, p->stream, [&]() -> int {
        int64_t removed = 0;
        if (p->n > 0) {
            LB_HIP(hipSetDevice(p->device));
            hipStream_t s = p->stream;
            removed = remove_by_id(p->device, s, buf, n, labels, p->part.d_ids.get(), p->n, [&] { return ivf_removal_ready(p, vis, s); },
                                   [&](const uint32_t *d_cnt) { return ivf_commit_removed(p, d_cnt, vis, s); });
        }
        if (n_removed) *n_removed = removed;
        return LB_OK;
    });
}

// The entry points (the statement is include/longbow_gpu.h's, above lb_gpu_ivf_remove).  Argument checks answer before a device
// is touched.
inline int ivf_remove(IvfHandle *p, int64_t n, const int64_t *labels, int64_t *n_removed)
{
    if (!p || n < 0 || (n > 0 && !labels)) return LB_ERR_INVALID_ARG;
    if (n == 0) { if (n_removed) *n_removed = 0; return LB_OK; }
    std::unique_lock<std::shared_mutex> g(p->mu);
    return ivf_remove_labels(p, n, labels, n_removed);
}
inline int ivf_remove_rows(IvfHandle *p, int64_t n, const int64_t *rows, int64_t *n_removed)
{
    if (!p || n < 0 || (n > 0 && !rows)) return LB_ERR_INVALID_ARG;
    if (n == 0) { if (n_removed) *n_removed = 0; return LB_OK; }
    std::unique_lock<std::shared_mutex> g(p->mu);
    return ivf_remove_positions(p, n, rows, false, n_removed);
}
inline int ivf_remove_device(IvfHandle *p, int64_t n, const int64_t *d_labels, int64_t *n_removed)
{
    if (!p || n < 0 || (n > 0 && !d_labels)) return LB_ERR_INVALID_ARG;
    if (n == 0) { if (n_removed) *n_removed = 0; return LB_OK; }
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (!p->part.has_ids) return ivf_remove_positions(p, n, d_labels, true, n_removed);
    // ids: the set is sorted on the host (n is small beside ntotal, and this is on no search's path)
    std::vector<int64_t> host;
    const int rc = guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        host.resize((size_t)n);
        LB_HIP(hipMemcpy(host.data(), d_labels, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
        return LB_OK;
    });
    return rc != LB_OK ? rc : ivf_remove_labels(p, n, host.data(), n_removed);
}
inline int64_t ivf_nlive(const IvfHandle *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<IvfHandle *>(p)->mu);
    return p->n - p->n_dead;
}
inline int64_t ivf_ndeleted(const IvfHandle *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<IvfHandle *>(p)->mu);
    return p->n_dead;
}

// Compaction of a handle whose rows are row_bytes each (any element type; a code handle's rows are its codes in insertion order)
// at rows(), which is called under the handle's lock.  Everything that can be refused happens before the first row
// moves: every buffer and lease, the survivor list, the survivors' assignments gathered into a scratch, the new lists sorted from
// it into the pair not in use, their sizes read back and checked.  Then the rounds (lb_remove.h) move rows, ids and, under a
// caller's filter, the mask bytes; relist(nxt, nlive, s) enqueues what the handle derives from the moved rows and the new lists
// d_list[nxt] (the list-major codes of a handle with `positions`: into buffers that exist at `capacity` already, so it allocates
// nothing and refuses nothing; the others pass ivf_no_relist); the assignments are copied in, `live` is reset, the visible lists
// of a surviving filter are built from the new lists, and the commit comes last.  No row is assigned again: its list moves with it.
inline void ivf_no_relist(int, int64_t, hipStream_t) {}
template <class Rows, class Relist> int ivf_compact(IvfHandle *p, Rows &&rows, size_t row_bytes, int64_t *old_rows, int64_t cap, Relist &&relist)
{
    if (!p) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(p->mu);
    IvfPartition &P = p->part;
    const int64_t n_old = p->n, nlive = p->n - p->n_dead;
    if (old_rows && cap < nlive) {
        p->set_error("old_rows has room for %lld rows, the handle holds %lld live ones", (long long)cap, (long long)nlive);
        return LB_ERR_INVALID_ARG;
    }
    if (p->n_dead == 0) { // nothing to do: every row stays where it is
        if (old_rows)
            for (int64_t j = 0; j < nlive; j++) old_rows[j] = j;
        return LB_OK;
    }
    // the survivor list, launch_compact_mask's scratch, a round's rows, the survivors' assignments, the sort's and the visible lists'
    Lease lmap, lscr, lgather, lassign, hist, vis;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        RowFilter &f = p->filter;
        const bool keep_filter = f.on && p->has_filter; // a caller's filter survives, its bytes move with the rows
        const size_t idb = P.has_ids ? sizeof(int64_t) : 0, mb = keep_filter ? 1 : 0;
        const int64_t R = std::min<int64_t>(compact_round_rows(row_bytes + idb + mb), std::max<int64_t>(nlive, 1));
        const int nxt = 1 - P.cur, vto = 1 - p->vcur;
        // 0. every buffer before the first launch
        char *gx = nullptr, *gi = nullptr, *gm = nullptr;
        lease_layout(lgather, p->device, [&](Carve cv) {
            gx = cv.take<char>((size_t)R * row_bytes);
            gi = cv.take<char>((size_t)R * idb);
            gm = cv.take<char>((size_t)R * mb);
            return cv.off;
        });
        lassign.reset(p->device, (size_t)std::max<int64_t>(nlive, 1) * sizeof(uint32_t));
        hist.reset(p->device, ivf_sort_hist_words(nlive, P.nlist) * 4);
        if (keep_filter) {
            if (p->d_vlist[vto].count() < (size_t)p->capacity) p->d_vlist[vto].alloc((size_t)p->capacity);
            vis.reset(p->device, ivf_visible_scratch_bytes(nlive));
        }
        std::vector<uint32_t> hmap(old_rows ? (size_t)nlive : 0);
        std::vector<int64_t> sizes, vsizes;
        // 1. the ascending survivor list, map[j] >= j, and the first removed row
        int64_t first = 0;
        if (const int rc = compact_survivors(p, p->device, p->live.get(), n_old, nlive, lmap, lscr, hmap, &first, s)) return rc;
        const uint32_t *map = lmap.as<uint32_t>();
        // 2. the survivors' lists, in their new order; 3. the lists over them, into the pair not in use; 4. their sizes, checked
        uint32_t *d_newassign = lassign.as<uint32_t>();
        launch_gather_rows(P.d_assign.get(), map, nlive, sizeof(uint32_t), d_newassign, p->device, s);
        LB_HIP(launch_ivf_sort(d_newassign, nlive, P.nlist, hist.as<uint32_t>(), P.d_off[nxt].get(), P.d_list[nxt].get(), s));
        if (const int rc = ivf_read_lists(p, P, nlive, sizes, s)) return rc;
        // 5. the rows move, in place: from here on nothing but a device fault fails the call
        const CompactArray arrays[3] = {{rows(), row_bytes, gx}, {P.d_ids.get(), idb, gi}, {f.mask.get(), mb, gm}};
        compact_walk(arrays, 3, map, first, nlive, R, p->device, s);
        relist(nxt, nlive, s);
        if (nlive > 0) {
            LB_HIP(hipMemcpyAsync(P.d_assign.get(), d_newassign, (size_t)nlive * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            LB_HIP(hipMemsetAsync(p->live.get(), 0xff, (size_t)nlive, s));
        }
        int64_t nvis = 0;
        if (keep_filter) { // the row list and the visible lists of the mask where it now lies, from the new lists
            f.rebuild(nlive, s);
            nvis = ivf_build_visible(p, P.all_lists(nxt), nlive, vto, vis, vsizes, s);
            if (nvis != f.n_visible) throw std::logic_error("the visible lists do not hold the visible rows");
        }
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        // 6. commit
        P.h_sizes.swap(sizes);
        P.cur = nxt;
        p->n = nlive;
        p->n_dead = 0;
        f.live = nullptr;
        f.on = keep_filter; // (without a caller's filter there is no mask any more)
        p->has_filter = keep_filter;
        if (keep_filter) ivf_commit_visible(p, vsizes, nvis);
        for (int64_t j = 0; j < (int64_t)hmap.size(); j++) old_rows[j] = (int64_t)hmap[(size_t)j];
        return LB_OK;
    });
}

// ---- a row bitmap given with the search call ------------------------------------------------------------------------------
// The bitmap as an entry point got it: host or device memory, one bit per row position, least significant bit first.  Without
// `bits` there is none: the plain search.
struct CallBitmap {
    const uint8_t *bits = nullptr;
    int64_t nbits = 0, stride = 0;
    bool on_device = false;
};

// The call's filter as the search loop takes it.  mode, rowof, rowof_len: what the entries of the handle's lists are (lb_ivf.h,
// IVF_CALL_*), filled by call_filter from the handle.
struct IvfCallFilter {
    const uint8_t *d_bits = nullptr; // device memory; query q of the call reads d_bits + q stride
    int64_t stride = 0, nbits = 0;
    bool on = false;
    int mode = IVF_CALL_ROWS;
    const uint32_t *rowof = nullptr;
    uint32_t rowof_len = 0;
};

// The call's filter from its bitmap, under the reader lock and before anything is launched: the refusals (set_filter's n != ntotal
// rule, and the stride), then a host bitmap's bytes go into `lease` (the caller's, declared outside its guard) ahead of the
// search on s.
inline int call_filter(IvfHandle *p, int64_t nq, const CallBitmap &b, Lease &lease, hipStream_t s, IvfCallFilter &f)
{
    f = IvfCallFilter{};
    if (!b.bits) return LB_OK;
    if (b.nbits < 0 || b.nbits != p->n) {
        p->set_error("a bitmap of %lld bits for %lld rows", (long long)b.nbits, (long long)p->n);
        return LB_ERR_INVALID_ARG;
    }
    const int64_t bytes = (b.nbits + 7) / 8;
    if (b.stride < 0 || (b.stride > 0 && b.stride < bytes)) {
        p->set_error("bitmap stride %lld: 0 (one bitmap for every query) or at least the %lld bytes of %lld bits", (long long)b.stride,
                     (long long)bytes, (long long)b.nbits);
        return LB_ERR_INVALID_ARG;
    }
    if (bytes == 0) return LB_OK; // (an empty handle: all padding with or without it)
    f.d_bits = b.bits;
    if (!b.on_device) {
        const size_t total = (size_t)(b.stride > 0 ? (nq - 1) * b.stride : 0) + (size_t)bytes;
        lease.reset(p->device, total);
        LB_HIP(hipMemcpyAsync(lease.p, b.bits, total, hipMemcpyHostToDevice, s));
        f.d_bits = lease.as<uint8_t>();
    }
    f.stride = b.stride;
    f.nbits = b.nbits;
    f.on = true;
    if (p->positions) { // the lists of all rows hold rows, the visible ones positions into them (IvfHandle)
        f.mode = p->filter.on ? IVF_CALL_POS_VISIBLE : IVF_CALL_POS_ALL;
        f.rowof = p->part.d_list[p->part.cur].get();
        f.rowof_len = (uint32_t)p->n;
    }
    return LB_OK;
}

// The call's lists in the search loop: the probed lists of the handle's lists L, compacted under the bitmap into synthetic lists
// (lb_ivf.h: offsets, probes and 4 bytes of rows per key) that the plan, the middle steps and the selection walk in place of L and
// of the coarse search's probes.  The host keeps sizing by the sizes of L, and nothing comes back to it in between.
// The per-slot form: behind the probes of each batch launch_ivf_call_lists compacts the lists that batch probes.
// The shared form: under ONE bitmap (stride 0), when the call's nq * pmax exceeds the rows of all lists of L, the per-slot form
// would walk more list positions than L holds.  Then every list of L is compacted once, in the first batch: launch_ivf_call_lists
// over one pseudo-query that probes lists 0 .. nlist - 1, pmax being the rows of all lists (at least 1), which leaves list l as
// synthetic list 2 l; each batch only renames its probes (launch_ivf_call_shared_probes).  The rule is the host's, from numbers it
// has; the synthetic list of a probe holds the same entries in the same order in both forms, so the result does not depend on
// which ran.
struct IvfCallWalk {
    const IvfCallFilter &f;
    bool shared = false;
    int64_t all_rows = 1;
    IvfCallLists cl{};
    int64_t *d_ident = nullptr, *d_renamed = nullptr; // shared: the pseudo-query's probes; a batch's renamed probes

    // n: the handle's rows (both list arrays hold room for every row, all of it written or allocated)
    IvfCallWalk(const IvfCallFilter &filter, const IvfLists &L, const std::vector<int64_t> &sizes, int64_t n, int64_t nq, int64_t pmax) : f(filter)
    {
        if (!f.on) return;
        int64_t rows = 0;
        for (const int64_t v : sizes) rows += v;
        shared = f.stride == 0 && nq * pmax > rows;
        all_rows = std::max<int64_t>(rows, 1);
        cl.L = L;
        cl.rows_len = (uint32_t)n;
        cl.mode = f.mode;
        cl.rowof = f.rowof;
        cl.rowof_len = f.rowof_len;
        cl.stride = f.stride;
        cl.nbits = f.nbits;
    }
    // the synthetic lists' pieces of the scratch, for batches of nb queries at np probes
    void layout(Carve &c, int64_t nb, int np, int64_t pmax)
    {
        const size_t nlist = (size_t)cl.L.nlist;
        if (shared) {
            cl.soff = c.take<uint32_t>((nlist * 2 + 1) * 4);
            cl.sprobes = c.take<int64_t>(nlist * 8);
            d_ident = c.take<int64_t>(nlist * 8);
            d_renamed = c.take<int64_t>((size_t)nb * np * 8);
            cl.srows = c.take<uint32_t>((size_t)all_rows * 4);
        } else if (f.on) {
            cl.soff = c.take<uint32_t>(((size_t)nb * np * 2 + 1) * 4);
            cl.sprobes = c.take<int64_t>((size_t)nb * np * 8);
            cl.srows = c.take<uint32_t>((size_t)nb * pmax * 4);
        }
    }
    // Enqueues the lists of the batch `a` (its queries from q0 of the call on, d_probes the coarse search's) and points a.L and
    // a.probes at them; -> the entries of their row array
    int64_t batch(IvfBatch &a, int64_t q0, const int64_t *d_probes, hipStream_t s)
    {
        if (shared) { // every list once, in the first batch; then this batch's probes by the lists' new numbers
            if (q0 == 0) {
                cl.probes = d_ident;
                cl.nq = 1;
                cl.np = cl.L.nlist;
                cl.pmax = all_rows;
                cl.bits = f.d_bits;
                launch_ivf_all_probes(d_ident, 1, cl.L.nlist, s);
                launch_ivf_call_lists(cl, s);
            }
            launch_ivf_call_shared_probes(d_probes, (int64_t)a.nq * a.np, cl.L.nlist, d_renamed, s);
            a.probes = d_renamed;
        } else { // the probed lists of this batch, slot by slot
            cl.probes = d_probes;
            cl.nq = a.nq;
            cl.np = a.np;
            cl.pmax = a.pmax;
            cl.bits = f.d_bits + (size_t)q0 * f.stride;
            launch_ivf_call_lists(cl, s);
            a.probes = cl.sprobes;
        }
        a.L = cl.lists();
        return shared ? all_rows : (int64_t)a.nq * a.pmax;
    }
};

// ---- the search loop --------------------------------------------------------------------------------------------------------
// One search call: nq device-resident queries of element type Q, k, nprobe, where the results go, the stream, the context, the
// lease the scratch goes into (the caller's, declared outside its guard) and the call's filter.
template <class Q> struct IvfCallOf {
    int64_t nq;
    const Q *queries;
    int k, nprobe;
    float *dist;
    int64_t *labels;
    hipStream_t s;
    const lb_cancel *ctx;
    Lease &sc;
    IvfCallFilter filter;
};
using IvfCall = IvfCallOf<float>; // what the loop takes: every handle's coarse search reads f32 queries

// A handle's fixed choices.  timing[slots] (under err_mu) gets the ms of a profiled search summed over its batches: probes, plan
// (up to middle's first next()), a slot per further next(), selection.  batch_cap: queries per batch at most, for a handle whose own
// scratch grows with the batch (the residual IVF-PQ handle's tables).  select: the selection's launcher, for a handle whose keys
// are not pack_entry's (the integer keys of IVF-SQ8 and IVF-BQ); launch_ivf_select's arguments and meaning.
using IvfSelectFn = void (*)(const IvfBatch &, int, const int64_t *, float *, int64_t *, hipStream_t);
struct IvfSearchForm {
    float *timing;
    int slots;
    int64_t batch_cap = kQueryBatch;
    IvfSelectFn select = launch_ivf_select;
};

// What a batch's middle steps are told beside the batch itself
struct IvfWalk {
    int64_t maxlen;        // the longest list of the handle
    bool subset;           // the batch walks other lists than those of all rows: the visible ones, or the call's
    int64_t entries;       // the entries of the row array behind the lists it walks; with `positions` they are positions, which a
                           // scan bounds by this (the `_visible` scans' nvis)
    IvfLists own;          // the handle's lists and the coarse search's probes, whatever the batch walks (the residual IVF-PQ handle
    const int64_t *probes; // subtracts the centroid of the list probed)
};

// Exact k-NN of the call's queries among the rows of their probed lists, the lists being h->lists(); the caller holds the reader
// lock, has made the device current and has checked the arguments.  Per batch: the probes, the call's lists if it has a filter,
// launch_ivf_plan, the handle's middle steps, the selection.
//   extra(c, a, nb)           sets the handle's own fields of the batch a (a.D is set) and take()s its scratch pieces for a batch
//                             of nb queries from the Carve c (it runs twice)
//   middle(a, w, poll, next)  enqueues what fills a.keys; poll() is false once ctx fired, next() ends a timing slot and then polls;
//                             after either's false it enqueues nothing more and returns false
// Profiling costs a drain per batch.  The launches of the call's lists fall into the plan's timing slot.
template <class Extra, class Middle> int ivf_search(IvfHandle *h, const IvfCall &c, const IvfSearchForm &form, Extra &&extra, Middle &&middle)
{
    if (const int st = ivf_live_ok(h)) return st;
    IvfPartition &P = h->part;
    const std::vector<int64_t> &sizes = h->sizes();
    const int64_t nq = c.nq;
    hipStream_t s = c.s;
    int64_t st[4] = {nq, 0, 0, 0};
    auto publish = [&]() {
        std::lock_guard<std::mutex> g(h->err_mu);
        std::copy(st, st + 4, P.stats);
    };
    if (h->n == 0) { // all padding, without a launch
        LB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.dist), 0x7f7fffff /* FLT_MAX */, (size_t)nq * c.k, s));
        LB_HIP(hipMemsetAsync(c.labels, 0xff, (size_t)nq * c.k * 8, s));
        LB_HIP(hipStreamSynchronize(s));
        publish();
        return LB_OK;
    }
    const int np = std::min(c.nprobe, P.nlist);
    // pmax: the rows a query can scan at most, the sum of the np largest lists
    std::vector<int64_t> big(sizes);
    std::partial_sort(big.begin(), big.begin() + np, big.end(), std::greater<int64_t>());
    int64_t pmax = 0;
    for (int i = 0; i < np; i++) pmax += big[i];
    pmax = std::max<int64_t>(pmax, 1);
    const int64_t nb = std::min(std::min(nq, std::max<int64_t>(1, std::min(form.batch_cap, kQueryBatch))), std::max<int64_t>(1, kKeyScratch / 8 / pmax));
    IvfBatch a{};
    a.D = h->dims;
    a.L = h->lists();
    a.np = np;
    a.pmax = pmax;
    IvfWalk w{big[0], h->filter.on, h->filter.on ? h->filter.n_visible : h->n, a.L, nullptr};
    IvfCallWalk calls(c.filter, a.L, sizes, h->n, nq, pmax);
    int64_t *d_probes = nullptr;
    float *d_pdist = nullptr;
    unsigned long long *d_stats = nullptr;
    auto layout = [&](Carve cv) {
        a.probes = w.probes = d_probes = cv.take<int64_t>((size_t)nb * np * 8);
        d_pdist = cv.take<float>((size_t)nb * np * 4);
        a.seg = cv.take<uint32_t>((size_t)nb * (np + 1) * 4);
        d_stats = cv.take<unsigned long long>(4 * 8);
        calls.layout(cv, nb, np, pmax);
        extra(cv, a, nb);
        a.keys = cv.take<uint64_t>((size_t)nb * pmax * 8);
        return cv.off;
    };
    lease_layout(c.sc, h->device, layout);
    int cancelled = 0;
    auto go = [&]() { // false: the context fired, nothing more is enqueued
        cancelled = ctx_state(c.ctx);
        return cancelled == 0;
    };
    if (go()) LB_HIP(hipMemsetAsync(d_stats, 0, 4 * 8, s));
    const bool prof = P.profiling.load();
    const int slots = form.slots;
    EventH ev[kMaxTimingSlots + 1];
    float tms[kMaxTimingSlots] = {0, 0, 0, 0, 0};
    if (prof)
        for (int i = 0; i <= slots; i++) LB_HIP(hipEventCreate(&ev[i].h));
    int e = 0; // the next event of the batch
    auto mark = [&]() { if (prof) LB_HIP(hipEventRecord(ev[e++], s)); };
    auto next = [&]() { mark(); return go(); };
    for (int64_t q0 = 0; q0 < nq && !cancelled; q0 += nb) {
        a.nq = (int)std::min(nb, nq - q0);
        a.Q = c.queries + (size_t)q0 * h->dims;
        e = 0;
        mark();
        // the probes (the inner index polls ctx before its own launches).  More than LB_MAX_K of them is more than the coarse
        // search returns: with every list probed they are all the lists, and their order does not reach the result
        if (np == P.nlist && np > LB_MAX_K) launch_ivf_all_probes(d_probes, a.nq, np, s);
        else if (const int rc = lb_gpu_index_search_device_ctx(P.coarse, a.nq, a.Q, np, d_pdist, d_probes, s, c.ctx)) return coarse_fail(h, P, rc, s);
        if (!next()) break;
        if (c.filter.on) { // the lists under the call's bitmap: everything below walks those
            if (!go()) break;
            w.subset = true;
            w.entries = calls.batch(a, q0, d_probes, s);
        }
        launch_ivf_plan(a, d_stats, s);
        if (!middle(a, w, go, next)) break;
        if (!next()) break;
        form.select(a, c.k, P.has_ids ? P.d_ids.get() : nullptr, c.dist + (size_t)q0 * c.k, c.labels + (size_t)q0 * c.k, s);
        mark();
        if (prof) {
            LB_HIP(hipEventSynchronize(ev[slots]));
            for (int i = 0; i < slots; i++) {
                float ms = 0.f;
                LB_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
                tms[i] += ms;
            }
        }
    }
    LB_LAUNCH_CHECK();
    unsigned long long h_stats[4] = {0, 0, 0, 0};
    if (!cancelled) LB_HIP(hipMemcpyAsync(h_stats, d_stats, sizeof h_stats, hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    if (cancelled) return ctx_fail(h, cancelled);
    for (int i = 1; i < 4; i++) st[i] = (int64_t)h_stats[i];
    publish();
    if (prof) {
        std::lock_guard<std::mutex> g(h->err_mu);
        std::copy(tms, tms + slots, form.timing);
    }
    return LB_OK;
}

// ---- the entry points -------------------------------------------------------------------------------------------------------
// T: a handle with `part` and `timing[]`.  dev(p, c) is the handle's call of ivf_search for the call c (an IvfCallOf<Q>).  Argument
// checks answer before a device is touched.
template <class T>
int ivf_search_args(T *p, int64_t nq, const void *queries, int k, int nprobe, const void *dist, const void *labels, const lb_cancel *ctx)
{
    return knn_args(p, nq, queries, k, dist, labels, ctx, [&]() -> int {
        const int nlist = p->part.nlist;
        if (nprobe <= 0) {
            p->set_error("nprobe=%d: at least one list is probed", nprobe);
            return LB_ERR_INVALID_ARG;
        }
        if (nprobe < nlist && nprobe > LB_MAX_K) { // (more probes than the coarse search returns)
            p->set_error("nprobe=%d: fewer than all %d lists are at most %d probes", nprobe, nlist, LB_MAX_K);
            return LB_ERR_UNSUPPORTED;
        }
        return LB_OK;
    });
}

// the call as a record, its filter from the bitmap (`bits`: the caller's lease, declared outside its guard), then the handle's search
template <class T, class Q, class Dev>
int ivf_search_call(T *p, int64_t nq, const Q *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels, hipStream_t s, const lb_cancel *ctx,
                    Lease &sc, const CallBitmap &bitmap, Lease &bits, Dev &&dev)
{
    IvfCallOf<Q> c{nq, d_queries, k, nprobe, d_dist, d_labels, s, ctx, sc, {}};
    if (const int st = call_filter(p, nq, bitmap, bits, s, c.filter)) return st;
    return dev(p, c);
}

// Q: the queries' element type, f32 but for the IVF-Flat handle over int8 rows.  bitmap: a row bitmap given with the call, if any
template <class T, class Q, class Dev>
int ivf_search_device_ctx(T *p, int64_t nq, const Q *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels, void *stream,
                          const lb_cancel *ctx, Dev &&dev, const CallBitmap &bitmap = CallBitmap{})
{
    const int rc = ivf_search_args(p, nq, d_queries, k, nprobe, d_dist, d_labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    Lease sc, bits;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        return ivf_search_call(p, nq, d_queries, k, nprobe, d_dist, d_labels, s, ctx, sc, bitmap, bits, dev);
    });
}

template <class T, class Q, class Dev>
int ivf_search_ctx(T *p, int64_t nq, const Q *queries, int k, int nprobe, float *dist, int64_t *labels, const lb_cancel *ctx, Dev &&dev,
                   const CallBitmap &bitmap = CallBitmap{})
{
    const int rc = ivf_search_args(p, nq, queries, k, nprobe, dist, labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    Lease bits;
    return host_knn(
        p, nq, (size_t)p->dims * sizeof(Q), k, dist, labels,
        [&](Lease &dq, Lease &, hipStream_t s) { LB_HIP(hipMemcpyAsync(dq.p, queries, (size_t)nq * p->dims * sizeof(Q), hipMemcpyHostToDevice, s)); },
        [&](Lease &dq, float *d_dist, int64_t *d_labels, hipStream_t s, Lease &sc) {
            return ivf_search_call(p, nq, dq.as<Q>(), k, nprobe, d_dist, d_labels, s, ctx, sc, bitmap, bits, dev);
        });
}

template <class T> int ivf_list_sizes(T *p, int64_t *sizes)
{
    if (!p || !sizes) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    std::copy(p->part.h_sizes.begin(), p->part.h_sizes.end(), sizes);
    return LB_OK;
}

template <class T> int ivf_assignments(T *p, int64_t row0, int64_t n, int32_t *lists)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !lists)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        LB_HIP(hipMemcpy(lists, p->part.d_assign.get() + row0, (size_t)n * 4, hipMemcpyDeviceToHost)); // (list numbers are below 2^16)
        return LB_OK;
    });
}

template <class T> int ivf_get_centroids(T *p, float *out)
{
    if (!p || !out) return LB_ERR_INVALID_ARG;
    std::copy(p->part.h_cent.begin(), p->part.h_cent.end(), out); // (fixed at creation)
    return LB_OK;
}

template <class T> int ivf_last_search_stats(T *p, int64_t out[4])
{
    if (!p || !out) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->err_mu);
    std::copy(p->part.stats, p->part.stats + 4, out);
    return LB_OK;
}

template <class T> int ivf_set_profiling(T *p, int enable)
{
    if (!p) return LB_ERR_INVALID_ARG;
    p->part.profiling.store(enable != 0);
    return LB_OK;
}

inline int ivf_last_build_timing(IvfHandle *p, float *ms)
{
    if (!p || !ms) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->err_mu);
    *ms = p->build_ms;
    return LB_OK;
}

template <class T> int ivf_last_timing(T *p, float *ms)
{
    if (!p || !ms) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->err_mu);
    std::copy(std::begin(p->timing), std::end(p->timing), ms);
    return LB_OK;
}

#pragma GCC visibility pop
} // namespace lb
