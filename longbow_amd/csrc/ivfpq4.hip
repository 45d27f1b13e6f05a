// ivfpq4.hip -- host side of the lb_gpu_ivfpq4_* entry points of include/longbow_gpu.h: the IVF-PQ4 index, the coarse partition
// of the IVF handles (lb_ivf_host.h) over the packed 4-bit codes of the PQ4 handle (pq4.hip, lb_pq4.h).  The new kernels are in
// kernels_ivfpq4.hip; the coarse quantiser is an inner exact f32 index over the centroids, the lists are kernels_ivf.hip's, the
// list-major copy and the residuals kernels_ivfpq.hip's, the codec kernels_pq4.hip's and the table kernels_pq.hip's at K = 16.
// A handle is plain or residual (lb_gpu_ivfpq4_new_residual), as ivfpq.hip's: a residual handle encodes a row less its list's
// centroid and searches under a table per probed list (ivfpq4_rsearch_dev); everything else is shared.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_ivf_host.h"
#include "lb_ivfpq4.h"

using namespace lb;

struct lb_gpu_ivfpq4 : IvfHandle { // the partition (L2), and under a row filter the visible lists of positions (lb_ivf_host.h)
    int M = 0, sub = 0, P = 0, order = 0; // P: bytes of a packed row
    DevBuf<float> d_codebooks;         // [M][16][sub]
    DevBuf<uint8_t> d_codes;           // [capacity][P], packed, insertion order: what get_codes unpacks
    // the list-major codes are built for all rows by every add, with the lists, into the pair that is not in use
    DevBuf<uint8_t> d_lcodes[2];       // [capacity][P]: lcodes[pos] = codes[list[pos]]
    bool residual = false;             // the codes are of res(row, list(row)) and a search builds a table per probed list; fixed at creation
    DevBuf<float> d_cent;              // [nlist][dims], a residual handle's own copy of the centroids
    float timing[5] = {0, 0, 0, 0, 0}; // of the last profiled search (under err_mu): probes, plan, tables, scan, select; ms summed over its batches
};

namespace {

uint32_t rd_u32le(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

void ivfpq4_grow(lb_gpu_ivfpq4 *p, int64_t need, bool want_ids)
{
    ivf_grow(p, need, want_ids, {{&p->d_codes, (size_t)p->P, false}, {p->d_lcodes, (size_t)p->P, true}});
}

// what the handle derives from new lists (an add's, a compaction's): the packed codes in list order, into the pair not in use
// (launch_ivfpq_permute moves rows of any byte width: 16-byte pieces when P % 16 == 0, else single bytes)
auto ivfpq4_relist(lb_gpu_ivfpq4 *p)
{
    return [p](int nxt, int64_t total, hipStream_t s) {
        launch_ivfpq_permute(p->d_codes.get(), p->part.d_list[nxt].get(), total, p->P, p->d_lcodes[nxt].get(), s);
    };
}

// The handle's share of the add (lb_ivf_host.h: ivf_add), as ivfpq.hip's: a piece's rows, on a residual handle less their lists'
// centroids (`res`), are encoded and packed straight into d_codes.
int add_impl(lb_gpu_ivfpq4 *p, int64_t n, const float *vectors, const int64_t *ids, bool on_device)
{
    if (!p) return LB_ERR_INVALID_ARG;
    IvfAddSource src{vectors, on_device, p->device, p->dims};
    Lease res;
    return ivf_add(
        p, n, vectors, ids, on_device, piece_rows(p->dims), [&](int64_t total, bool want_ids) { ivfpq4_grow(p, total, want_ids); }, src,
        [&](const float *d_rows, int64_t r0, int64_t cnt, int64_t piece, hipStream_t s) {
            if (p->residual) {
                if (r0 == 0) res.reset(p->device, (size_t)piece * p->dims * 4);
                launch_ivfpq_residual_rows(d_rows, p->part.d_assign.get() + p->n + r0, p->d_cent.get(), cnt, p->dims, p->part.nlist, res.as<float>(), s);
                d_rows = res.as<float>();
            }
            launch_pq4_encode(p->d_codebooks.get(), p->M, p->sub, d_rows, cnt, p->d_codes.get() + (size_t)(p->n + r0) * p->P, true, s);
        },
        ivfpq4_relist(p));
}

// The residual handle's call of the search loop, shaped like ivfpq.hip's ivfpq_rsearch_dev: the middle steps run over the pairs
// (query, slot) of the batch, the residual queries and their tables in one timing slot, then the scan.  A table is M * 64 bytes,
// so the batch rule (ivfpq4_table_plan over kTableScratch) rarely binds: at M = 96 the budget holds 174,762 tables, a full batch
// of 1024 queries at 170 probes.  Rounds of slots, where one query's tables do not fit, go as there.
constexpr int64_t kTableLaunch = 65535; // pairs a launch_build_adc_table call takes: its queries are on grid.y

int ivfpq4_rsearch_dev(lb_gpu_ivfpq4 *p, const IvfCall &c)
{
    const IvfPartition &P = p->part;
    const uint8_t *lcodes = p->d_lcodes[P.cur].get();
    const int np = std::min(c.nprobe, P.nlist);
    const IvfpqTablePlan tp = ivfpq4_table_plan(np, p->M, kTableScratch);
    const size_t tab = (size_t)p->M * PQ4_K; // floats a table
    float *d_rq = nullptr, *d_tables = nullptr;
    uint32_t *d_items = nullptr; // the scan's work list, where it runs from one (ivfpq_rscan_plan)
    hipStream_t s = c.s;
    return ivf_search(
        p, c, IvfSearchForm{p->timing, 5, tp.nb},
        [&](Carve &cv, IvfBatch &, int64_t nb) {
            const size_t pairs = (size_t)nb * (size_t)tp.slots; // of a round
            d_rq = cv.take<float>(pairs * p->dims * 4);
            d_tables = cv.take<float>(pairs * tab * 4);
            d_items = cv.take<uint32_t>((pairs + 1) * 4);
        },
        [&](const IvfBatch &b, const IvfWalk &w, auto &&poll, auto &&next) {
            if (!next()) return false; // (the plan's slot ends here)
            for (int s0 = 0; s0 < np; s0 += (int)tp.slots) {
                const int ns = (int)std::min<int64_t>(tp.slots, np - s0);
                const int64_t pairs = (int64_t)b.nq * ns;
                if (s0 > 0 && !poll()) return false;
                IvfBatch rb = b; // (a table belongs to the list probed, whatever the batch walks)
                rb.L = w.own;
                rb.probes = w.probes;
                launch_ivfpq_residual_queries(rb, s0, ns, p->d_cent.get(), d_rq, s);
                for (int64_t p0 = 0; p0 < pairs; p0 += kTableLaunch) {
                    if (!poll()) return false;
                    launch_build_adc_table(p->d_codebooks.get(), p->M, PQ4_K, p->sub, d_rq + (size_t)p0 * p->dims,
                                           (int)std::min(kTableLaunch, pairs - p0), d_tables + (size_t)p0 * tab, s);
                }
                if (s0 == 0 ? !next() : !poll()) return false;
                if (w.subset) launch_ivfpq4_rscan_visible(b, s0, ns, d_tables, p->M, lcodes, p->n, w.maxlen, d_items, P.d_list[P.cur].get(), w.entries, s);
                else launch_ivfpq4_rscan(b, s0, ns, d_tables, p->M, lcodes, p->n, w.maxlen, d_items, s);
            }
            return true;
        });
}

// The handle's call of the search loop (lb_ivf_host.h): exact ADC k-NN.  Its middle steps are the queries' tables, a timing slot
// of their own, and the scan of the list-major codes: over the lists of all rows by position, or, where the batch walks the
// visible lists or a call's (w.subset), in its `_visible` form over their entries, positions bounded by w.entries.
int ivfpq4_search_dev(lb_gpu_ivfpq4 *p, const IvfCall &c)
{
    if (p->residual) return ivfpq4_rsearch_dev(p, c);
    const IvfPartition &P = p->part;
    const uint8_t *lcodes = p->d_lcodes[P.cur].get();
    float *d_tables = nullptr;
    hipStream_t s = c.s;
    return ivf_search(
        p, c, IvfSearchForm{p->timing, 5},
        [&](Carve &cv, IvfBatch &, int64_t nb) { d_tables = cv.take<float>((size_t)nb * p->M * PQ4_K * 4); },
        [&](const IvfBatch &b, const IvfWalk &w, auto &&, auto &&next) {
            if (!next()) return false; // (the plan's slot ends here)
            launch_build_adc_table(p->d_codebooks.get(), p->M, PQ4_K, p->sub, b.Q, b.nq, d_tables, s);
            if (!next()) return false;
            if (w.subset) launch_ivfpq4_scan_visible(b, d_tables, p->M, lcodes, p->n, P.d_list[P.cur].get(), w.entries, s);
            else launch_ivfpq4_scan(b, d_tables, p->M, lcodes, p->n, s);
            return true;
        });
}

// both constructors: the same arguments, limits, order of checks and status codes (ivfpq.hip's, with K = 16 and PQ4_MAX_M)
lb_gpu_ivfpq4 *ivfpq4_new(int device, const uint8_t *blob, size_t len, int order, int nlist, const float *centroids, int *out_status, bool residual)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    // the blob, as lb_gpu_pq_new reads it (DeserializePQEncoder, internal/pq/persistence.go:38-73)
    if (!blob || len < 12 || order < 0 || order > 1 || nlist <= 0 || !centroids) { st(LB_ERR_INVALID_ARG); return nullptr; }
    const uint32_t dims = rd_u32le(blob), M = rd_u32le(blob + 4), K = rd_u32le(blob + 8);
    if (M == 0 || dims % M != 0) { st(LB_ERR_INVALID_ARG); return nullptr; }
    const size_t sub = dims / M;
    if (len != 12 + (size_t)M * K * sub * 4) { st(LB_ERR_INVALID_ARG); return nullptr; }
    if (K != (uint32_t)PQ4_K || M > (uint32_t)PQ4_MAX_M || dims > LB_MAX_DIM || nlist > IVF_MAX_NLIST) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    return ivf_open<lb_gpu_ivfpq4>(device, (int)dims, 0 /* L2 */, order, nlist, centroids, out_status, [&](lb_gpu_ivfpq4 *p) {
        p->M = (int)M;
        p->sub = (int)sub;
        p->P = pq4_row_bytes((int)M);
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

lb_gpu_ivfpq4 *lb_gpu_ivfpq4_new(int device, const uint8_t *blob, size_t len, int order, int nlist, const float *centroids, int *out_status)
{
    return ivfpq4_new(device, blob, len, order, nlist, centroids, out_status, false);
}
lb_gpu_ivfpq4 *lb_gpu_ivfpq4_new_residual(int device, const uint8_t *blob, size_t len, int order, int nlist, const float *centroids,
                                          int *out_status)
{
    return ivfpq4_new(device, blob, len, order, nlist, centroids, out_status, true);
}
int lb_gpu_ivfpq4_residual(const lb_gpu_ivfpq4 *p) { return p && p->residual ? 1 : 0; }

void lb_gpu_ivfpq4_free(lb_gpu_ivfpq4 *p) { handle_free(p); }
const char *lb_gpu_ivfpq4_last_error(const lb_gpu_ivfpq4 *p) { return handle_last_error(p); }
int lb_gpu_ivfpq4_dims(const lb_gpu_ivfpq4 *p) { return p ? p->dims : 0; }
int lb_gpu_ivfpq4_m(const lb_gpu_ivfpq4 *p) { return p ? p->M : 0; }
int lb_gpu_ivfpq4_order(const lb_gpu_ivfpq4 *p) { return p ? p->order : 0; }
int lb_gpu_ivfpq4_nlist(const lb_gpu_ivfpq4 *p) { return p ? p->part.nlist : 0; }
int64_t lb_gpu_ivfpq4_ntotal(const lb_gpu_ivfpq4 *p) { return handle_ntotal(p); }

int64_t lb_gpu_ivfpq4_hbm_bytes(const lb_gpu_ivfpq4 *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_ivfpq4 *>(p)->mu);
    return (int64_t)(p->d_codes.count() + p->d_lcodes[0].count() + p->d_lcodes[1].count() + (p->d_codebooks.count() + p->d_cent.count()) * 4) + p->visible_bytes() +
           p->part.hbm_bytes();
}

int lb_gpu_ivfpq4_reserve(lb_gpu_ivfpq4 *p, int64_t n_total)
{
    return handle_reserve(p, n_total, [](lb_gpu_ivfpq4 *h, int64_t need) { ivfpq4_grow(h, need, h->part.has_ids); });
}

// M bytes a row, each below 16, as lb_gpu_pq4_get_codes: unpacked on the device into a pooled buffer, in pieces
int lb_gpu_ivfpq4_get_codes(lb_gpu_ivfpq4 *p, int64_t row0, int64_t n, uint8_t *codes)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !codes)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    Lease out;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        const int64_t piece = std::min<int64_t>(n, std::max<int64_t>(1, ((int64_t)256 << 20) / p->M));
        out.reset(p->device, (size_t)piece * p->M);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            launch_pq4_unpack(p->d_codes.get() + (size_t)(row0 + r0) * p->P, p->M, cnt, out.as<uint8_t>(), p->stream);
            LB_LAUNCH_CHECK();
            LB_HIP(hipMemcpyAsync(codes + (size_t)r0 * p->M, out.p, (size_t)cnt * p->M, hipMemcpyDeviceToHost, p->stream));
            LB_HIP(hipStreamSynchronize(p->stream)); // (the buffer is filled again)
        }
        return LB_OK;
    });
}

// ---- the row filter (lb_handle.h, lb_ivf_host.h) ------------------------------------------------------------------------
int64_t lb_gpu_ivfpq4_nvisible(const lb_gpu_ivfpq4 *p) { return filter_nvisible(p); }
int lb_gpu_ivfpq4_set_filter(lb_gpu_ivfpq4 *p, const uint8_t *mask, int64_t n) { return ivf_set_filter(p, mask, n); }
int lb_gpu_ivfpq4_filter_int64(lb_gpu_ivfpq4 *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                               int64_t validity_offset, int combine)
{
    return ivf_filter_column<int64_t>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivfpq4_filter_float32(lb_gpu_ivfpq4 *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                                 int64_t validity_offset, int combine)
{
    return ivf_filter_column<float>(p, column, n, value, op, validity, validity_offset, combine);
}
int lb_gpu_ivfpq4_last_build_timing(lb_gpu_ivfpq4 *p, float *ms) { return ivf_last_build_timing(p, ms); }

// ---- removal and compaction (lb_ivf_host.h, lb_remove.h) ----------------------------------------------------------------
int lb_gpu_ivfpq4_remove(lb_gpu_ivfpq4 *p, int64_t n, const int64_t *labels, int64_t *n_removed) { return ivf_remove(p, n, labels, n_removed); }
int lb_gpu_ivfpq4_remove_device(lb_gpu_ivfpq4 *p, int64_t n, const int64_t *d_labels, int64_t *n_removed)
{
    return ivf_remove_device(p, n, d_labels, n_removed);
}
int lb_gpu_ivfpq4_remove_rows(lb_gpu_ivfpq4 *p, int64_t n, const int64_t *rows, int64_t *n_removed) { return ivf_remove_rows(p, n, rows, n_removed); }
int64_t lb_gpu_ivfpq4_nlive(const lb_gpu_ivfpq4 *p) { return ivf_nlive(p); }
int64_t lb_gpu_ivfpq4_ndeleted(const lb_gpu_ivfpq4 *p) { return ivf_ndeleted(p); }
// (the packed codes in insertion order are the rows that move, P bytes each; the list-major copy of the pair not in use is written
// from them and the new lists, as an add writes it: no row is encoded again, a residual code included)
int lb_gpu_ivfpq4_compact(lb_gpu_ivfpq4 *p, int64_t *old_rows, int64_t cap)
{
    if (!p) return LB_ERR_INVALID_ARG;
    return ivf_compact(p, [p] { return static_cast<void *>(p->d_codes.get()); }, (size_t)p->P, old_rows, cap, ivfpq4_relist(p));
}

// ---- what the IVF handles share (lb_ivf_host.h) -------------------------------------------------------------------------
int lb_gpu_ivfpq4_add(lb_gpu_ivfpq4 *p, int64_t n, const float *vectors, const int64_t *ids) { return add_impl(p, n, vectors, ids, false); }
int lb_gpu_ivfpq4_add_device(lb_gpu_ivfpq4 *p, int64_t n, const float *d_vectors, const int64_t *d_ids) { return add_impl(p, n, d_vectors, d_ids, true); }
int lb_gpu_ivfpq4_get_centroids(lb_gpu_ivfpq4 *p, float *out) { return ivf_get_centroids(p, out); }
int lb_gpu_ivfpq4_list_sizes(lb_gpu_ivfpq4 *p, int64_t *sizes) { return ivf_list_sizes(p, sizes); }
int lb_gpu_ivfpq4_assignments(lb_gpu_ivfpq4 *p, int64_t row0, int64_t n, int32_t *lists) { return ivf_assignments(p, row0, n, lists); }
int lb_gpu_ivfpq4_search_device_ctx(lb_gpu_ivfpq4 *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels,
                                    void *stream, const lb_cancel *ctx)
{
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, ivfpq4_search_dev);
}
int lb_gpu_ivfpq4_search_ctx(lb_gpu_ivfpq4 *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels,
                             const lb_cancel *ctx)
{
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, ivfpq4_search_dev);
}
int lb_gpu_ivfpq4_search(lb_gpu_ivfpq4 *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels)
{
    return lb_gpu_ivfpq4_search_ctx(p, nq, queries, k, nprobe, dist, labels, nullptr);
}
// the same searches under a row bitmap given with the call (a NULL bitmap: the plain search), plain and residual handles alike
int lb_gpu_ivfpq4_search_bitmap_device_ctx(lb_gpu_ivfpq4 *p, int64_t nq, const float *d_queries, int k, int nprobe, const uint8_t *d_bitmap,
                                           int64_t nbits, int64_t stride_bytes, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    return ivf_search_device_ctx(p, nq, d_queries, k, nprobe, d_dist, d_labels, stream, ctx, ivfpq4_search_dev,
                                 CallBitmap{d_bitmap, nbits, stride_bytes, true});
}
int lb_gpu_ivfpq4_search_bitmap_ctx(lb_gpu_ivfpq4 *p, int64_t nq, const float *queries, int k, int nprobe, const uint8_t *bitmap, int64_t nbits,
                                    int64_t stride_bytes, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    return ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, ctx, ivfpq4_search_dev, CallBitmap{bitmap, nbits, stride_bytes, false});
}
int lb_gpu_ivfpq4_last_search_stats(lb_gpu_ivfpq4 *p, int64_t out[4]) { return ivf_last_search_stats(p, out); }
int lb_gpu_ivfpq4_set_profiling(lb_gpu_ivfpq4 *p, int enable) { return ivf_set_profiling(p, enable); }
int lb_gpu_ivfpq4_last_timing(lb_gpu_ivfpq4 *p, float ms[5]) { return ivf_last_timing(p, ms); }

} // extern "C"
