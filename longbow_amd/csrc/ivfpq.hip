// ivfpq.hip -- host side of the lb_gpu_ivfpq_* entry points of include/longbow_gpu.h: the IVF-PQ index, the coarse partition of
// the IVF-Flat handle (ivf.hip) over the codes of the PQ handle (pq.hip).  The new kernels are in kernels_ivfpq.hip; the coarse
// quantiser is an inner exact f32 index over the centroids, the lists are kernels_ivf.hip's, the codec and the table
// kernels_pq.hip's and kernels_pq2.hip's.  A handle is plain or residual (lb_gpu_ivfpq_new_residual): a residual handle encodes a
// row less its list's centroid and searches under a table per probed list (ivfpq_rsearch_dev); everything else is shared.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_ivf_host.h"
#include "lb_ivfpq.h"

using namespace lb;

struct lb_gpu_ivfpq : IvfHandle { // the partition (L2), and under a row filter the visible lists of positions (lb_ivf_host.h)
    int M = 0, K = 0, sub = 0, order = 0;
    DevBuf<float> d_codebooks;      // [M][K][sub]
    DevBuf<uint8_t> d_codes;        // [capacity][M], insertion order: what get_codes returns
    // the list-major codes are built for all rows by every add, with the lists, into the pair that is not in use
    DevBuf<uint8_t> d_lcodes[2];    // [capacity][M]: lcodes[pos] = codes[list[pos]]
    bool residual = false;          // the codes are of res(row, list(row)) and a search builds a table per probed list; fixed at creation
    DevBuf<float> d_cent;           // [nlist][dims], a residual handle's own copy of the centroids (the coarse index keeps its rows to itself)
    float timing[5] = {0, 0, 0, 0, 0}; // of the last profiled search (under err_mu): probes, plan, tables, scan, select; ms summed over its batches (residual: ivfpq_rsearch_dev)
};

namespace {

uint32_t rd_u32le(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// All or nothing: every new buffer is allocated and filled before the first one replaces an old one.
void ivfpq_grow(lb_gpu_ivfpq *p, int64_t need, bool want_ids)
{
    const int64_t cap = ivf_grow_to(p, p->part, need, want_ids, (size_t)p->M); // 1.
    if (cap < 0) return;
    IvfGrowth g;                                                                // 2.
    DevBuf<uint8_t> nc, nlc[2];
    const int cur = p->part.cur;
    g.stage(p, cap, want_ids);
    if (g.resize) {
        nc.alloc((size_t)cap * p->M);
        for (DevBuf<uint8_t> &l : nlc) l.alloc((size_t)cap * p->M);
        if (p->n > 0) {
            LB_HIP(hipMemcpy(nc.get(), p->d_codes.get(), (size_t)p->n * p->M, hipMemcpyDeviceToDevice));
            LB_HIP(hipMemcpy(nlc[cur].get(), p->d_lcodes[cur].get(), (size_t)p->n * p->M, hipMemcpyDeviceToDevice));
        }
        p->filter.grow(p->n, cap);                                              // 3. (the last step that can fail)
    }
    g.commit(p);                                                                // 4.
    if (!g.resize) return;
    p->d_codes = std::move(nc);
    for (int i = 0; i < 2; i++) p->d_lcodes[i] = std::move(nlc[i]);
    p->capacity = cap;
}

// The vectors are assigned and encoded in pieces of piece_rows(dims) rows (64 Mi floats: 256 MB of host vectors staged at a time,
// 12 bytes of labels and distances a row of a piece) and are not kept.  Codes and lists of the new rows are written behind the
// stored ones, where they belong to nobody until the commit.
int add_impl(lb_gpu_ivfpq *p, int64_t n, const float *vectors, const int64_t *ids, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    IvfPartition &P = p->part;
    if (const int st = ivf_ids_consistent(p, P, ids)) return st;
    if (const int st = rows_fit(p, p->n, n)) return st;
    Lease vec, lab, hist, vis, res;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        const int64_t total = p->n + n;
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        std::vector<int64_t> sizes, vsizes;
        const bool filtered = p->filter.on;
        ivfpq_grow(p, total, ids != nullptr);
        if (ids) LB_HIP(hipMemcpyAsync(P.d_ids.get() + p->n, ids, (size_t)n * 8, kind, s));
        // 1. the vectors, a piece at a time: 2. their lists, 3. their codes
        const int64_t piece = std::min(n, piece_rows(p->dims));
        lab.reset(p->device, ivf_assign_bytes(piece));
        if (!on_device) vec.reset(p->device, (size_t)piece * p->dims * 4);
        if (p->residual) res.reset(p->device, (size_t)piece * p->dims * 4);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            const float *d_new = vectors + (size_t)r0 * p->dims;
            if (!on_device) {
                LB_HIP(hipMemcpyAsync(vec.p, d_new, (size_t)cnt * p->dims * 4, hipMemcpyHostToDevice, s));
                d_new = vec.as<float>();
            }
            if (const int rc = ivf_assign(p, P, p->n + r0, cnt, d_new, lab, s)) return rc;
            if (p->residual) { // the piece's rows less their lists' centroids are what is encoded
                launch_ivfpq_residual_rows(d_new, P.d_assign.get() + p->n + r0, p->d_cent.get(), cnt, p->dims, P.nlist, res.as<float>(), s);
                d_new = res.as<float>();
            }
            launch_pq_encode(p->d_codebooks.get(), p->M, p->K, p->sub, d_new, cnt, p->d_codes.get() + (size_t)(p->n + r0) * p->M, s);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(s)); // (the staging buffer and the labels are reused by the next piece)
        }
        // 4. the lists of all rows and 5. their codes in list order, into the pair not in use
        const int nxt = 1 - P.cur;
        ivf_add_live(p, total, s); // (a handle that has removed rows: the new ones are live)
        ivf_sort_lists(p, P, total, hist, s);
        launch_ivfpq_permute(p->d_codes.get(), P.d_list[nxt].get(), total, p->M, p->d_lcodes[nxt].get(), s);
        if (const int rc = ivf_read_lists(p, P, total, sizes, s)) return rc;
        // 6. under a filter the new rows are visible: the visible lists of all rows, from the new lists (every position changes
        //    with them), into the pair not in use
        const int64_t nvis = filtered ? ivf_add_visible(p, total, vis, vsizes, s) : 0;
        // 7. commit (nothing below throws)
        if (filtered) ivf_commit_visible(p, vsizes, nvis);
        P.h_sizes.swap(sizes);
        P.cur = nxt;
        P.has_ids = ids != nullptr;
        p->n = total;
        return LB_OK;
    });
}

// The residual handle's call of the search loop.  A query has a table per probed list, so the middle steps run over the pairs
// (query, slot) of the batch: the residual queries and their tables, in one timing slot, then the scan.  The batch is shrunk so
// that its nb * np tables fit kTableScratch (ivfpq_table_plan); only when one query's np tables do not, the middle steps go in
// rounds of slots, each residual queries -> tables -> scan of those slots, all into the one keys[q][.], and the selection runs
// once.  Timing: slot 3 is the first round's residual queries and tables, slot 4 its scan and every further round whole.
constexpr int64_t kTableLaunch = 65535; // pairs a launch_build_adc_table call takes: its queries are on grid.y

// Under a call's bitmap (filter.on) the batch's lists and probes are the call's synthetic ones, whose entries are positions: the
// scan takes its `_visible` form over them whether or not the handle has a filter, bounded by the entries of the call's row array,
// and the residual queries are built from a copy of the batch whose lists and probes are the handle's and the coarse search's
// (real_probes: where the batch pointed at layout time, the same buffer every batch), since a table belongs to the list probed.
int ivfpq_rsearch_dev(lb_gpu_ivfpq *p, const IvfBatch &a, int64_t nq, const float *d_Q, int k, int nprobe, float *d_dist, int64_t *d_labels,
                      hipStream_t s, const lb_cancel *ctx, Lease &sc, const IvfCallFilter &filter)
{
    const IvfPartition &P = p->part;
    const uint8_t *lcodes = p->d_lcodes[P.cur].get();
    const int np = std::min(nprobe, P.nlist);
    const IvfpqTablePlan tp = ivfpq_table_plan(np, p->M, kTableScratch);
    float *d_rq = nullptr, *d_tables = nullptr;
    uint32_t *d_items = nullptr; // the scan's work list, where it runs from one (ivfpq_rscan_plan)
    const int64_t *real_probes = nullptr;
    const IvfLists own = p->lists();
    return ivf_search(
        p, p->part, own, p->sizes(), a, nq, d_Q, k, nprobe, d_dist, d_labels, s, ctx, sc, p->timing, 5,
        [&](Carve &c, IvfBatch &b, int64_t nb) {
            real_probes = b.probes;
            const size_t pairs = (size_t)nb * (size_t)tp.slots; // of a round
            d_rq = c.take<float>(pairs * p->dims * 4);
            d_tables = c.take<float>(pairs * p->M * 256 * 4);
            d_items = c.take<uint32_t>((pairs + 1) * 4);
        },
        [&](const IvfBatch &b, int64_t maxlen, auto &&poll, auto &&next) {
            if (!next()) return false; // (the plan's slot ends here)
            for (int s0 = 0; s0 < np; s0 += (int)tp.slots) {
                const int ns = (int)std::min<int64_t>(tp.slots, np - s0);
                const int64_t pairs = (int64_t)b.nq * ns;
                if (s0 > 0 && !poll()) return false;
                IvfBatch rb = b;
                rb.L = own;
                rb.probes = real_probes;
                launch_ivfpq_residual_queries(rb, s0, ns, p->d_cent.get(), d_rq, s);
                for (int64_t p0 = 0; p0 < pairs; p0 += kTableLaunch) {
                    if (!poll()) return false;
                    launch_build_adc_table(p->d_codebooks.get(), p->M, p->K, p->sub, d_rq + (size_t)p0 * p->dims,
                                           (int)std::min(kTableLaunch, pairs - p0), d_tables + (size_t)p0 * p->M * 256, s);
                }
                if (s0 == 0 ? !next() : !poll()) return false;
                if (filter.on)
                    launch_ivfpq_rscan_visible(b, s0, ns, d_tables, p->M, lcodes, p->n, maxlen, d_items, P.d_list[P.cur].get(), filter.call_rows, s);
                else if (p->filter.on)
                    launch_ivfpq_rscan_visible(b, s0, ns, d_tables, p->M, lcodes, p->n, maxlen, d_items, P.d_list[P.cur].get(),
                                               p->filter.n_visible, s);
                else launch_ivfpq_rscan(b, s0, ns, d_tables, p->M, lcodes, p->n, maxlen, d_items, s);
            }
            return true;
        },
        tp.nb, launch_ivf_select, filter);
}

// The handle's call of the search loop (lb_ivf_host.h): exact ADC k-NN; under a filter it walks the visible lists.  Its middle steps
// are the queries' tables, a timing slot of their own, and the scan of the list-major codes.
// filter: the call's own row bitmap (the *_bitmap entry points): the scan then takes its `_visible` form over the call's lists of
// positions, as above.
int ivfpq_search_dev(lb_gpu_ivfpq *p, int64_t nq, const float *d_Q, int k, int nprobe, float *d_dist, int64_t *d_labels, hipStream_t s,
                     const lb_cancel *ctx, Lease &sc, const IvfCallFilter &filter = IvfCallFilter{})
{
    if (const int st = ivf_live_ok(p)) return st;
    const IvfPartition &P = p->part;
    IvfBatch a{};
    a.X = nullptr; // (only the plan and the selection take the batch as the IVF-Flat kernels do: neither reads rows)
    a.D = p->dims;
    const uint8_t *lcodes = p->d_lcodes[P.cur].get();
    float *d_tables = nullptr;
    if (p->residual) return ivfpq_rsearch_dev(p, a, nq, d_Q, k, nprobe, d_dist, d_labels, s, ctx, sc, filter);
    return ivf_search(
        p, p->part, p->lists(), p->sizes(), a, nq, d_Q, k, nprobe, d_dist, d_labels, s, ctx, sc, p->timing, 5,
        [&](Carve &c, IvfBatch &, int64_t nb) { d_tables = c.take<float>((size_t)nb * p->M * 256 * 4); },
        [&](const IvfBatch &b, int64_t, auto &&, auto &&next) {
            if (!next()) return false; // (the plan's slot ends here)
            launch_build_adc_table(p->d_codebooks.get(), p->M, p->K, p->sub, b.Q, b.nq, d_tables, s);
            if (!next()) return false;
            if (filter.on) launch_ivfpq_scan_visible(b, d_tables, p->M, lcodes, p->n, P.d_list[P.cur].get(), filter.call_rows, s);
            else if (p->filter.on) launch_ivfpq_scan_visible(b, d_tables, p->M, lcodes, p->n, P.d_list[P.cur].get(), p->filter.n_visible, s);
            else launch_ivfpq_scan(b, d_tables, p->M, lcodes, p->n, s);
            return true;
        },
        kQueryBatch, launch_ivf_select, filter);
}

// the search under a row bitmap given with the call: lb_ivf_host.h's refusals and copy, then the search above
int ivfpq_search_bitmap_dev(lb_gpu_ivfpq *p, int64_t nq, const float *d_Q, int k, int nprobe, float *d_dist, int64_t *d_labels, hipStream_t s,
                            const lb_cancel *ctx, Lease &sc, const CallBitmap &b, Lease &bits)
{
    IvfCallFilter f;
    if (const int st = call_filter(p, nq, b, bits, s, f)) return st;
    return ivfpq_search_dev(p, nq, d_Q, k, nprobe, d_dist, d_labels, s, ctx, sc, f);
}

// both constructors: the same arguments, limits, order of checks and status codes
lb_gpu_ivfpq *ivfpq_new(int device, const uint8_t *blob, size_t len, int order, int nlist, const float *centroids, int *out_status, bool residual)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    // the blob, as lb_gpu_pq_new reads it (DeserializePQEncoder, internal/pq/persistence.go:38-73)
    if (!blob || len < 12 || order < 0 || order > 1 || nlist <= 0 || !centroids) { st(LB_ERR_INVALID_ARG); return nullptr; }
    const uint32_t dims = rd_u32le(blob), M = rd_u32le(blob + 4), K = rd_u32le(blob + 8);
    if (M == 0 || dims % M != 0) { st(LB_ERR_INVALID_ARG); return nullptr; }
    const size_t sub = dims / M;
    if (len != 12 + (size_t)M * K * sub * 4) { st(LB_ERR_INVALID_ARG); return nullptr; }
    if (K != 256 || (size_t)M * 256 * 4 > 160 * 1024 - 1024 || dims > LB_MAX_DIM || nlist > IVF_MAX_NLIST) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    return ivf_open<lb_gpu_ivfpq>(device, (int)dims, 0 /* L2 */, order, nlist, centroids, out_status, [&](lb_gpu_ivfpq *p) {
        p->M = (int)M;
        p->K = (int)K;
        p->sub = (int)sub;
        p->order = order;
        p->positions = true; // a visible list addresses the list-major codes
        p->d_codebooks.alloc((len - 12) / sizeof(float));
        LB_HIP(hipMemcpy(p->d_codebooks.get(), blob + 12, len - 12, hipMemcpyHostToDevice)); // (f32 little-endian on the wire, as pq.hip)
        p->residual = residual;
        if (residual) {
            p->d_cent.alloc((size_t)nlist * dims);
            LB_HIP(hipMemcpy(p->d_cent.get(), centroids, (size_t)nlist * dims * 4, hipMemcpyHostToDevice));
        }
    });
}

} // namespace

extern "C" {

lb_gpu_ivfpq *lb_gpu_ivfpq_new(int device, const uint8_t *blob, size_t len, int order, int nlist, const float *centroids, int *out_status)
{
    return ivfpq_new(device, blob, len, order, nlist, centroids, out_status, false);
}
lb_gpu_ivfpq *lb_gpu_ivfpq_new_residual(int device, const uint8_t *blob, size_t len, int order, int nlist, const float *centroids,
                                        int *out_status)
{
    return ivfpq_new(device, blob, len, order, nlist, centroids, out_status, true);
}
int lb_gpu_ivfpq_residual(const lb_gpu_ivfpq *p) { return p && p->residual ? 1 : 0; }

void lb_gpu_ivfpq_free(lb_gpu_ivfpq *p) { handle_free(p); }
const char *lb_gpu_ivfpq_last_error(const lb_gpu_ivfpq *p) { return handle_last_error(p); }
int lb_gpu_ivfpq_dims(const lb_gpu_ivfpq *p) { return p ? p->dims : 0; }
int lb_gpu_ivfpq_m(const lb_gpu_ivfpq *p) { return p ? p->M : 0; }
int lb_gpu_ivfpq_order(const lb_gpu_ivfpq *p) { return p ? p->order : 0; }
int lb_gpu_ivfpq_nlist(const lb_gpu_ivfpq *p) { return p ? p->part.nlist : 0; }
int64_t lb_gpu_ivfpq_ntotal(const lb_gpu_ivfpq *p) { return handle_ntotal(p); }

int64_t lb_gpu_ivfpq_hbm_bytes(const lb_gpu_ivfpq *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_ivfpq *>(p)->mu);
    return (int64_t)(p->d_codes.count() + p->d_lcodes[0].count() + p->d_lcodes[1].count() + (p->d_codebooks.count() + p->d_cent.count()) * 4) + p->visible_bytes() +
           p->part.hbm_bytes();
}

int lb_gpu_ivfpq_reserve(lb_gpu_ivfpq *p, int64_t n_total)
{
    return handle_reserve(p, n_total, [](lb_gpu_ivfpq *h, int64_t need) { ivfpq_grow(h, need, h->part.has_ids); });
}

int lb_gpu_ivfpq_get_codes(lb_gpu_ivfpq *p, int64_t row0, int64_t n, uint8_t *codes)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        LB_HIP(hipMemcpy(codes, p->d_codes.get() + (size_t)row0 * p->M, (size_t)n * p->M, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- the row filter (lb_handle.h, lb_ivf_host.h) ------------------------------------------------------------------------
int64_t lb_gpu_ivfpq_nvisible(const lb_gpu_ivfpq *p) { return filter_nvisible(p); }
int lb_gpu_ivfpq_set_filter(lb_gpu_ivfpq *p, const uint8_t *mask, int64_t n) { return ivf_set_filter(p, mask, n); }
int lb_gpu_ivfpq_filter_int64(lb_gpu_ivfpq *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                              int64_t validity_offset, int combine)
{
    return ivf_filter_column<int64_t>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivfpq_filter_float32(lb_gpu_ivfpq *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                                int64_t validity_offset, int combine)
{
    return ivf_filter_column<float>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivfpq_last_build_timing(lb_gpu_ivfpq *p, float *ms) { return ivf_last_build_timing(p, ms); }

// ---- removal and compaction (lb_ivf_host.h, lb_remove.h) ----------------------------------------------------------------
int lb_gpu_ivfpq_remove(lb_gpu_ivfpq *p, int64_t n, const int64_t *labels, int64_t *n_removed) { return ivf_remove(p, n, labels, n_removed); }
int lb_gpu_ivfpq_remove_device(lb_gpu_ivfpq *p, int64_t n, const int64_t *d_labels, int64_t *n_removed)
{
    return ivf_remove_device(p, n, d_labels, n_removed);
}
int lb_gpu_ivfpq_remove_rows(lb_gpu_ivfpq *p, int64_t n, const int64_t *rows, int64_t *n_removed) { return ivf_remove_rows(p, n, rows, n_removed); }
int64_t lb_gpu_ivfpq_nlive(const lb_gpu_ivfpq *p) { return ivf_nlive(p); }
int64_t lb_gpu_ivfpq_ndeleted(const lb_gpu_ivfpq *p) { return ivf_ndeleted(p); }
// (the codes in insertion order are the rows that move, M bytes each; the list-major copy of the pair not in use is written from
// them and the new lists, as an add writes it, before the commit flips part.cur: no row is encoded again, a residual code included,
// for the list it was taken against moves with it)
int lb_gpu_ivfpq_compact(lb_gpu_ivfpq *p, int64_t *old_rows, int64_t cap)
{
    if (!p) return LB_ERR_INVALID_ARG;
    return ivf_compact(p, [p] { return static_cast<void *>(p->d_codes.get()); }, (size_t)p->M, old_rows, cap, [p](int nxt, int64_t nlive, hipStream_t s) {
        launch_ivfpq_permute(p->d_codes.get(), p->part.d_list[nxt].get(), nlive, p->M, p->d_lcodes[nxt].get(), s);
    });
}

// ---- what the IVF handles share (lb_ivf_host.h) -------------------------------------------------------------------------
int lb_gpu_ivfpq_add(lb_gpu_ivfpq *p, int64_t n, const float *vectors, const int64_t *ids) { return add_impl(p, n, vectors, ids, false); }
int lb_gpu_ivfpq_add_device(lb_gpu_ivfpq *p, int64_t n, const float *d_vectors, const int64_t *d_ids) { return add_impl(p, n, d_vectors, d_ids, true); }
int lb_gpu_ivfpq_get_centroids(lb_gpu_ivfpq *p, float *out) { return ivf_get_centroids(p, out); }
int lb_gpu_ivfpq_list_sizes(lb_gpu_ivfpq *p, int64_t *sizes) { return ivf_list_sizes(p, sizes); }
int lb_gpu_ivfpq_assignments(lb_gpu_ivfpq *p, int64_t row0, int64_t n, int32_t *lists) { return ivf_assignments(p, row0, n, lists); }
int lb_gpu_ivfpq_search_device_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels,
                                   void *stream, const lb_cancel *ctx)
{
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, [](auto &&...args) { return ivfpq_search_dev(args...); });
}
int lb_gpu_ivfpq_search_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                            const lb_cancel *ctx)
{
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, [](auto &&...args) { return ivfpq_search_dev(args...); });
}
int lb_gpu_ivfpq_search(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels)
{
    return lb_gpu_ivfpq_search_ctx(p, nq, queries, k, nprobe, dist, labels, nullptr);
}
// the same searches under a row bitmap given with the call (a NULL bitmap: the plain search), plain and residual handles alike
int lb_gpu_ivfpq_search_bitmap_device_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                          int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    Lease bits;
    const CallBitmap b{d_bitmap, nbits, stride_bytes, true};
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx,
                                 [&](auto &&...args) { return ivfpq_search_bitmap_dev(args..., b, bits); });
}
int lb_gpu_ivfpq_search_bitmap_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, const uint8_t *bitmap, int64_t nbits,
                                   int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    Lease bits;
    const CallBitmap b{bitmap, nbits, stride_bytes, false};
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, [&](auto &&...args) { return ivfpq_search_bitmap_dev(args..., b, bits); });
}
int lb_gpu_ivfpq_last_search_stats(lb_gpu_ivfpq *p, int64_t out[4]) { return ivf_last_search_stats(p, out); }
int lb_gpu_ivfpq_set_profiling(lb_gpu_ivfpq *p, int enable) { return ivf_set_profiling(p, enable); }
int lb_gpu_ivfpq_last_timing(lb_gpu_ivfpq *p, float ms[5]) { return ivf_last_timing(p, ms); }

} // extern "C"
