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

void ivfpq_grow(lb_gpu_ivfpq *p, int64_t need, bool want_ids)
{
    ivf_grow(p, need, want_ids, {{&p->d_codes, (size_t)p->M, false}, {p->d_lcodes, (size_t)p->M, true}});
}

// what the handle derives from new lists (an add's, a compaction's): the codes in list order, into the pair not in use
auto ivfpq_relist(lb_gpu_ivfpq *p)
{
    return [p](int nxt, int64_t total, hipStream_t s) {
        launch_ivfpq_permute(p->d_codes.get(), p->part.d_list[nxt].get(), total, p->M, p->d_lcodes[nxt].get(), s);
    };
}

// The handle's share of the add (lb_ivf_host.h: ivf_add).  The vectors are staged piece_rows(dims) rows at a time (64 Mi floats:
// 256 MB of host vectors, 12 bytes of labels and distances a row of a piece) and are not kept: a piece's codes are stored, on a
// residual handle those of the rows less their lists' centroids (`res`).
int add_impl(lb_gpu_ivfpq *p, int64_t n, const float *vectors, const int64_t *ids, bool on_device)
{
    if (!p) return LB_ERR_INVALID_ARG;
    IvfAddSource src{vectors, on_device, p->device, p->dims};
    Lease res;
    return ivf_add(
        p, n, vectors, ids, on_device, piece_rows(p->dims), [&](int64_t total, bool want_ids) { ivfpq_grow(p, total, want_ids); }, src,
        [&](const float *d_rows, int64_t r0, int64_t cnt, int64_t piece, hipStream_t s) {
            if (p->residual) {
                if (r0 == 0) res.reset(p->device, (size_t)piece * p->dims * 4);
                launch_ivfpq_residual_rows(d_rows, p->part.d_assign.get() + p->n + r0, p->d_cent.get(), cnt, p->dims, p->part.nlist, res.as<float>(), s);
                d_rows = res.as<float>();
            }
            launch_pq_encode(p->d_codebooks.get(), p->M, p->K, p->sub, d_rows, cnt, p->d_codes.get() + (size_t)(p->n + r0) * p->M, s);
        },
        ivfpq_relist(p));
}

// The residual handle's call of the search loop.  A query has a table per probed list, so the middle steps run over the pairs
// (query, slot) of the batch: the residual queries and their tables, in one timing slot, then the scan.  The batch is shrunk so
// that its nb * np tables fit kTableScratch (ivfpq_table_plan); only when one query's np tables do not, the middle steps go in
// rounds of slots, each residual queries -> tables -> scan of those slots, all into the one keys[q][.], and the selection runs
// once.  Timing: slot 3 is the first round's residual queries and tables, slot 4 its scan and every further round whole.
constexpr int64_t kTableLaunch = 65535; // pairs a launch_build_adc_table call takes: its queries are on grid.y

// The residual queries are built from a copy of the batch whose lists and probes are the handle's and the coarse search's (w.own,
// w.probes), whatever the batch walks, since a table belongs to the list probed.
int ivfpq_rsearch_dev(lb_gpu_ivfpq *p, const IvfCall &c)
{
    const IvfPartition &P = p->part;
    const uint8_t *lcodes = p->d_lcodes[P.cur].get();
    const int np = std::min(c.nprobe, P.nlist);
    const IvfpqTablePlan tp = ivfpq_table_plan(np, p->M, kTableScratch);
    float *d_rq = nullptr, *d_tables = nullptr;
    uint32_t *d_items = nullptr; // the scan's work list, where it runs from one (ivfpq_rscan_plan)
    hipStream_t s = c.s;
    return ivf_search(
        p, c, IvfSearchForm{p->timing, 5, tp.nb},
        [&](Carve &cv, IvfBatch &, int64_t nb) {
            const size_t pairs = (size_t)nb * (size_t)tp.slots; // of a round
            d_rq = cv.take<float>(pairs * p->dims * 4);
            d_tables = cv.take<float>(pairs * p->M * 256 * 4);
            d_items = cv.take<uint32_t>((pairs + 1) * 4);
        },
        [&](const IvfBatch &b, const IvfWalk &w, auto &&poll, auto &&next) {
            if (!next()) return false; // (the plan's slot ends here)
            for (int s0 = 0; s0 < np; s0 += (int)tp.slots) {
                const int ns = (int)std::min<int64_t>(tp.slots, np - s0);
                const int64_t pairs = (int64_t)b.nq * ns;
                if (s0 > 0 && !poll()) return false;
                IvfBatch rb = b;
                rb.L = w.own;
                rb.probes = w.probes;
                launch_ivfpq_residual_queries(rb, s0, ns, p->d_cent.get(), d_rq, s);
                for (int64_t p0 = 0; p0 < pairs; p0 += kTableLaunch) {
                    if (!poll()) return false;
                    launch_build_adc_table(p->d_codebooks.get(), p->M, p->K, p->sub, d_rq + (size_t)p0 * p->dims,
                                           (int)std::min(kTableLaunch, pairs - p0), d_tables + (size_t)p0 * p->M * 256, s);
                }
                if (s0 == 0 ? !next() : !poll()) return false;
                if (w.subset) launch_ivfpq_rscan_visible(b, s0, ns, d_tables, p->M, lcodes, p->n, w.maxlen, d_items, P.d_list[P.cur].get(), w.entries, s);
                else launch_ivfpq_rscan(b, s0, ns, d_tables, p->M, lcodes, p->n, w.maxlen, d_items, s);
            }
            return true;
        });
}

// The handle's call of the search loop (lb_ivf_host.h): exact ADC k-NN.  Its middle steps are the queries' tables, a timing slot
// of their own, and the scan of the list-major codes: over the lists of all rows by position, or, where the batch walks the
// visible lists or a call's (w.subset), in its `_visible` form over their entries, positions bounded by w.entries.
int ivfpq_search_dev(lb_gpu_ivfpq *p, const IvfCall &c)
{
    if (p->residual) return ivfpq_rsearch_dev(p, c);
    const IvfPartition &P = p->part;
    const uint8_t *lcodes = p->d_lcodes[P.cur].get();
    float *d_tables = nullptr;
    hipStream_t s = c.s;
    return ivf_search(
        p, c, IvfSearchForm{p->timing, 5},
        [&](Carve &cv, IvfBatch &, int64_t nb) { d_tables = cv.take<float>((size_t)nb * p->M * 256 * 4); },
        [&](const IvfBatch &b, const IvfWalk &w, auto &&, auto &&next) {
            if (!next()) return false; // (the plan's slot ends here)
            launch_build_adc_table(p->d_codebooks.get(), p->M, p->K, p->sub, b.Q, b.nq, d_tables, s);
            if (!next()) return false;
            if (w.subset) launch_ivfpq_scan_visible(b, d_tables, p->M, lcodes, p->n, P.d_list[P.cur].get(), w.entries, s);
            else launch_ivfpq_scan(b, d_tables, p->M, lcodes, p->n, s);
            return true;
        });
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
    return ivf_compact(p, [p] { return static_cast<void *>(p->d_codes.get()); }, (size_t)p->M, old_rows, cap, ivfpq_relist(p));
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
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, ivfpq_search_dev);
}
int lb_gpu_ivfpq_search_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                            const lb_cancel *ctx)
{
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, ivfpq_search_dev);
}
int lb_gpu_ivfpq_search(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels)
{
    return lb_gpu_ivfpq_search_ctx(p, nq, queries, k, nprobe, dist, labels, nullptr);
}
// the same searches under a row bitmap given with the call (a NULL bitmap: the plain search), plain and residual handles alike
int lb_gpu_ivfpq_search_bitmap_device_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                          int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, ivfpq_search_dev,
                                 CallBitmap{d_bitmap, nbits, stride_bytes, true});
}
int lb_gpu_ivfpq_search_bitmap_ctx(lb_gpu_ivfpq *p, int64_t nq, const float *queries, int k, int nprobe, const uint8_t *bitmap, int64_t nbits,
                                   int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, ivfpq_search_dev, CallBitmap{bitmap, nbits, stride_bytes, false});
}
int lb_gpu_ivfpq_last_search_stats(lb_gpu_ivfpq *p, int64_t out[4]) { return ivf_last_search_stats(p, out); }
int lb_gpu_ivfpq_set_profiling(lb_gpu_ivfpq *p, int enable) { return ivf_set_profiling(p, enable); }
int lb_gpu_ivfpq_last_timing(lb_gpu_ivfpq *p, float ms[5]) { return ivf_last_timing(p, ms); }

} // extern "C"
