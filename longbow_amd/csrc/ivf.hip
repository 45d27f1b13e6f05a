// ivf.hip -- host side of the lb_gpu_ivf_* entry points of include/longbow_gpu.h: the IVF-Flat index the reference names as
// a plug-point (internal/store/pluggable_index.go:18-25,100-104; its adapter, pluggable_index_adapters.go:116-223, is a stub).
// The kernels are in kernels_ivf.hip; the coarse quantiser is an inner exact f32 index over the centroids.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_handle.h"
#include "lb_ivf.h"

#include <atomic>
#include <functional>
#include <stdexcept>
#include <vector>

using namespace lb;

struct lb_gpu_ivf : FilteredHandle { // searches and reads share mu; adds, reserve and the filter calls take it alone
    int metric = 0, order = 0, nlist = 0;
    lb_gpu_index *coarse = nullptr; // the centroids: same device, dim, metric and order
    std::vector<float> h_cent;      // [nlist][dims]
    DevBuf<float> d_rows;           // [capacity][dims], insertion order
    DevBuf<int64_t> d_ids;          // [capacity] when ids were given
    bool has_ids = false;
    DevBuf<uint32_t> d_assign;      // [capacity]: list of each row
    // the lists are built for all rows by every add, into the pair that is not in use: a failed add leaves the old ones
    DevBuf<uint32_t> d_off[2];      // [nlist + 1]
    DevBuf<uint32_t> d_list[2];     // [capacity]
    int cur = 0;
    std::vector<int64_t> h_sizes;   // [nlist]: sizes grids and scratch without a device round trip
    // the row filter (lb_handle.h): a search under one walks the visible lists, the rows of each list whose mask byte is
    // non-zero, in the list's order.  They are built by every filter call and by every add to a filtered handle, into the pair
    // that is not in use; filter.n_visible is d_voff[vcur][nlist].  filter.rowmap is rebuilt by the filter calls only and
    // nothing here reads it.
    DevBuf<uint32_t> d_voff[2];     // [nlist + 1]
    DevBuf<uint32_t> d_vlist[2];    // [capacity] from the first filter on
    int vcur = 0;
    std::vector<int64_t> h_vsizes;  // [nlist]: what h_sizes is to the lists
    int64_t stats[4] = {0, 0, 0, 0}; // of the last search (under err_mu)
    std::atomic<bool> profiling{false};
    float timing[4] = {0, 0, 0, 0};  // of the last profiled search (under err_mu): probes, plan, scan, select; ms summed over its batches
    float build_ms = 0;              // of the last profiled build of the visible lists (under err_mu): its launches alone
    ~lb_gpu_ivf() { lb_gpu_index_free(coarse); }
    IvfLists all_lists(int i) const { return IvfLists{d_off[i].get(), d_list[i].get(), nlist}; }
    // what a search walks, and the sizes that go with it
    IvfLists lists() const { return filter.on ? IvfLists{d_voff[vcur].get(), d_vlist[vcur].get(), nlist} : all_lists(cur); }
    const std::vector<int64_t> &sizes() const { return filter.on ? h_vsizes : h_sizes; }
};

namespace {

constexpr int64_t kQueryBatch = 1024;              // queries per batch at most
constexpr int64_t kKeyScratch = (int64_t)1 << 30;  // bytes of keys a batch may hold

void ivf_grow(lb_gpu_ivf *p, int64_t need, bool want_ids)
{
    const bool ids_missing = want_ids && p->d_ids.count() < (size_t)std::max<int64_t>(p->capacity, 1);
    if (need <= p->capacity && !ids_missing) return;
    const int64_t cap = need <= p->capacity ? p->capacity : grow_capacity(p->capacity, need, (size_t)p->dims * 4);
    DevBuf<int64_t> ni;
    if (want_ids) {
        ni.alloc((size_t)cap);
        if (p->n > 0 && p->has_ids) LB_HIP(hipMemcpy(ni.get(), p->d_ids.get(), (size_t)p->n * 8, hipMemcpyDeviceToDevice));
    }
    if (cap != p->capacity) {
        DevBuf<float> nr;
        DevBuf<uint32_t> na, nl0, nl1, nv0, nv1;
        nr.alloc((size_t)cap * p->dims);
        na.alloc((size_t)cap);
        nl0.alloc((size_t)cap);
        nl1.alloc((size_t)cap);
        if (p->filter.on) { // an active filter keeps its visible lists
            nv0.alloc((size_t)cap);
            nv1.alloc((size_t)cap);
        }
        if (p->n > 0) {
            LB_HIP(hipMemcpy(nr.get(), p->d_rows.get(), (size_t)p->n * p->dims * 4, hipMemcpyDeviceToDevice));
            LB_HIP(hipMemcpy(na.get(), p->d_assign.get(), (size_t)p->n * 4, hipMemcpyDeviceToDevice));
            LB_HIP(hipMemcpy((p->cur ? nl1 : nl0).get(), p->d_list[p->cur].get(), (size_t)p->n * 4, hipMemcpyDeviceToDevice));
        }
        if (p->filter.on && p->filter.n_visible > 0)
            LB_HIP(hipMemcpy((p->vcur ? nv1 : nv0).get(), p->d_vlist[p->vcur].get(), (size_t)p->filter.n_visible * 4, hipMemcpyDeviceToDevice));
        p->filter.grow(p->n, cap); // (the last step that can fail)
        if (p->filter.on) {
            p->d_vlist[0] = std::move(nv0);
            p->d_vlist[1] = std::move(nv1);
        }
        p->d_rows = std::move(nr);
        p->d_assign = std::move(na);
        p->d_list[0] = std::move(nl0);
        p->d_list[1] = std::move(nl1);
        p->capacity = cap;
    }
    if (want_ids) p->d_ids = std::move(ni);
}

// The visible lists of mask[0, n) over the lists `L` of those n rows, into pair `to`; drains s.  Nothing of the handle but that
// pair's buffers is written: the caller commits vsizes, `to` and the count it gets back.  scratch: a lease declared outside the
// caller's guard.
int64_t build_visible(lb_gpu_ivf *p, const IvfLists &L, int64_t n, int to, Lease &scratch, std::vector<int64_t> &vsizes, hipStream_t s)
{
    std::vector<uint32_t> h_voff((size_t)p->nlist + 1);
    vsizes.resize((size_t)p->nlist);
    if (p->d_vlist[to].count() < (size_t)p->capacity) p->d_vlist[to].alloc((size_t)p->capacity);
    scratch.reset(p->device, ivf_visible_scratch_bytes(n));
    const bool prof = p->profiling.load();
    EventH ev[2];
    if (prof) {
        for (EventH &e : ev) LB_HIP(hipEventCreate(&e.h));
        LB_HIP(hipEventRecord(ev[0], s));
    }
    LB_HIP(launch_ivf_visible(p->filter.mask.get(), L, n, scratch.p, p->d_voff[to].get(), p->d_vlist[to].get(), s));
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
    for (int l = 0; l < p->nlist; l++) vsizes[l] = (int64_t)h_voff[l + 1] - (int64_t)h_voff[l];
    return (int64_t)h_voff[p->nlist];
}

// what a filter call hands to the shell (lb_handle.h: `built`): the visible lists of the mask it has just written
auto visible_builder(lb_gpu_ivf *p, Lease &scratch)
{
    return [p, &scratch](hipStream_t s) {
        std::vector<int64_t> vsizes;
        const int to = 1 - p->vcur;
        const int64_t nv = build_visible(p, p->all_lists(p->cur), p->n, to, scratch, vsizes, s);
        if (nv != p->filter.n_visible) throw std::logic_error("the visible lists do not hold the visible rows"); // (LB_ERR_INTERNAL)
        p->h_vsizes.swap(vsizes);
        p->vcur = to;
    };
}

// the coarse index's own refusal becomes the handle's; what the call enqueued on s is drained before its pooled buffers go back
int coarse_fail(lb_gpu_ivf *p, int rc, hipStream_t s)
{
    (void)hipStreamSynchronize(s);
    if (rc == LB_ERR_CANCELLED || rc == LB_ERR_DEADLINE) return ctx_fail(p, rc);
    p->set_error("coarse quantiser: %s", lb_gpu_last_error(p->coarse));
    return rc;
}

int add_impl(lb_gpu_ivf *p, int64_t n, const float *vectors, const int64_t *ids, bool on_device)
{
    if (!p || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::unique_lock<std::shared_mutex> g(p->mu);
    if (p->n > 0 && (ids != nullptr) != p->has_ids) {
        p->set_error("ids are given on every add or on none: the handle's rows have %s", p->has_ids ? "ids" : "none");
        return LB_ERR_INVALID_ARG;
    }
    if (const int st = rows_fit(p, p->n, n)) return st;
    Lease lab, hist, vis;
    return guard(p, p->stream, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        hipStream_t s = p->stream;
        const int64_t total = p->n + n;
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        std::vector<uint32_t> h_off((size_t)p->nlist + 1);
        std::vector<int64_t> sizes((size_t)p->nlist), vsizes;
        const bool filtered = p->filter.on;
        ivf_grow(p, total, ids != nullptr);
        // 1. the rows
        float *d_new = p->d_rows.get() + (size_t)p->n * p->dims;
        LB_HIP(hipMemcpyAsync(d_new, vectors, (size_t)n * p->dims * 4, kind, s));
        if (ids) LB_HIP(hipMemcpyAsync(p->d_ids.get() + p->n, ids, (size_t)n * 8, kind, s));
        // 2. their lists: the k = 1 search of each row over the centroids
        const size_t lb = up16((size_t)n * 8);
        lab.reset(p->device, lb + (size_t)n * 4);
        int64_t *d_lab = lab.as<int64_t>();
        float *d_dist = reinterpret_cast<float *>(lab.as<char>() + lb);
        if (const int rc = lb_gpu_index_search_device(p->coarse, n, d_new, 1, d_dist, d_lab, s)) return coarse_fail(p, rc, s);
        // 3. narrowed, 4. the lists of all rows, into the pair not in use
        launch_ivf_narrow(d_lab, n, p->d_assign.get() + p->n, s);
        const int nxt = 1 - p->cur;
        hist.reset(p->device, ivf_sort_hist_words(total, p->nlist) * 4);
        LB_HIP(launch_ivf_sort(p->d_assign.get(), total, p->nlist, hist.as<uint32_t>(), p->d_off[nxt].get(), p->d_list[nxt].get(), s));
        LB_LAUNCH_CHECK();
        LB_HIP(hipMemcpyAsync(h_off.data(), p->d_off[nxt].get(), h_off.size() * 4, hipMemcpyDeviceToHost, s));
        LB_HIP(hipStreamSynchronize(s));
        if ((int64_t)h_off[p->nlist] != total) {
            p->set_error("the lists hold %lld of %lld rows", (long long)h_off[p->nlist], (long long)total);
            return LB_ERR_INTERNAL;
        }
        for (int l = 0; l < p->nlist; l++) sizes[l] = (int64_t)h_off[l + 1] - (int64_t)h_off[l];
        // 5. under a filter the new rows are visible: the visible lists of all rows, from the new lists, into the pair not in use
        //    (the mask bytes behind the stored rows belong to nobody until the commit)
        const int vnxt = 1 - p->vcur;
        int64_t nvis = 0;
        if (filtered) {
            LB_HIP(hipMemsetAsync(p->filter.mask.get() + p->n, 1, (size_t)n, s));
            nvis = build_visible(p, p->all_lists(nxt), total, vnxt, vis, vsizes, s);
        }
        // 6. commit (nothing below throws)
        if (filtered) {
            p->h_vsizes.swap(vsizes);
            p->vcur = vnxt;
            p->filter.n_visible = nvis;
        }
        p->h_sizes.swap(sizes);
        p->cur = nxt;
        p->has_ids = ids != nullptr;
        p->n = total;
        return LB_OK;
    });
}

// Exact k-NN of nq device-resident queries among the rows of their probed lists; the caller holds the reader lock, has made the
// device current and has checked the arguments.  ctx is polled before every launch.  The scratch is leased into the caller's
// `sc`, declared outside the caller's guard as lb_handle.h asks of every pooled buffer.
int ivf_search_dev(lb_gpu_ivf *p, int64_t nq, const float *d_Q, int k, int nprobe, float *d_dist, int64_t *d_labels, hipStream_t s,
                   const lb_cancel *ctx, Lease &sc)
{
    int64_t st[4] = {nq, 0, 0, 0};
    auto publish = [&]() {
        std::lock_guard<std::mutex> g(p->err_mu);
        std::copy(st, st + 4, p->stats);
    };
    if (p->n == 0) { // all padding, without a launch
        LB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_dist), 0x7f7fffff /* FLT_MAX */, (size_t)nq * k, s));
        LB_HIP(hipMemsetAsync(d_labels, 0xff, (size_t)nq * k * 8, s));
        LB_HIP(hipStreamSynchronize(s));
        publish();
        return LB_OK;
    }
    const int np = std::min(nprobe, p->nlist);
    // pmax: the rows a query can scan at most, the sum of the np largest lists
    std::vector<int64_t> big(p->sizes()); // (the visible lists' under a filter)
    std::partial_sort(big.begin(), big.begin() + np, big.end(), std::greater<int64_t>());
    int64_t pmax = 0;
    for (int i = 0; i < np; i++) pmax += big[i];
    const int64_t maxlen = big[0];
    pmax = std::max<int64_t>(pmax, 1);
    const int64_t nb = std::min(std::min(nq, kQueryBatch), std::max<int64_t>(1, kKeyScratch / 8 / pmax));
    IvfBatch a{};
    a.X = p->d_rows.get();
    a.D = p->dims;
    a.L = p->lists();
    a.np = np;
    a.pmax = pmax;
    int64_t *d_probes = nullptr;
    float *d_pdist = nullptr, *d_qna = nullptr;
    unsigned long long *d_stats = nullptr;
    auto layout = [&](Carve c) {
        a.probes = d_probes = c.take<int64_t>((size_t)nb * np * 8);
        d_pdist = c.take<float>((size_t)nb * np * 4);
        a.seg = c.take<uint32_t>((size_t)nb * (np + 1) * 4);
        a.qna = d_qna = c.take<float>((size_t)nb * 4);
        d_stats = c.take<unsigned long long>(4 * 8);
        a.keys = c.take<uint64_t>((size_t)nb * pmax * 8);
        return c.off;
    };
    lease_layout(sc, p->device, layout);
    int cancelled = 0;
    auto go = [&]() { // false: the context fired, nothing more is enqueued
        cancelled = ctx_state(ctx);
        return cancelled == 0;
    };
    if (go()) LB_HIP(hipMemsetAsync(d_stats, 0, 4 * 8, s));
    // profiling: events between the steps, read after each batch (tools/ivf_bench.py); it costs a drain per batch
    const bool prof = p->profiling.load();
    EventH ev[5];
    float tms[4] = {0, 0, 0, 0};
    if (prof)
        for (EventH &e : ev) LB_HIP(hipEventCreate(&e.h));
    auto mark = [&](int i) { if (prof) LB_HIP(hipEventRecord(ev[i], s)); };
    for (int64_t q0 = 0; q0 < nq && !cancelled; q0 += nb) {
        a.nq = (int)std::min(nb, nq - q0);
        a.Q = d_Q + (size_t)q0 * p->dims;
        mark(0);
        // 1. the probes (the inner index polls ctx before its own launches).  More than LB_MAX_K of them is more than the coarse
        //    search returns: with every list probed they are all the lists, and their order does not reach the result
        if (np == p->nlist && np > LB_MAX_K) launch_ivf_all_probes(d_probes, a.nq, np, s);
        else if (const int rc = lb_gpu_index_search_device_ctx(p->coarse, a.nq, a.Q, np, d_pdist, d_probes, s, ctx)) return coarse_fail(p, rc, s);
        mark(1);
        if (!go()) break;
        launch_ivf_plan(a, d_stats, s);                                      // 2.
        if (p->metric == METRIC_COS) {
            if (!go()) break;
            launch_query_norms(p->order, a.Q, nullptr, a.nq, p->dims, d_qna, s);
        }
        mark(2);
        if (!go()) break;
        launch_ivf_scan(p->metric, p->order, a, maxlen, s);                  // 3.
        mark(3);
        if (!go()) break;
        launch_ivf_select(a, k, p->has_ids ? p->d_ids.get() : nullptr, d_dist + (size_t)q0 * k, d_labels + (size_t)q0 * k, s); // 4.
        mark(4);
        if (prof) {
            LB_HIP(hipEventSynchronize(ev[4]));
            for (int i = 0; i < 4; i++) {
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
    if (cancelled) return ctx_fail(p, cancelled);
    for (int i = 1; i < 4; i++) st[i] = (int64_t)h_stats[i];
    publish();
    if (prof) {
        std::lock_guard<std::mutex> g(p->err_mu);
        std::copy(tms, tms + 4, p->timing);
    }
    return LB_OK;
}

int search_args(lb_gpu_ivf *p, int64_t nq, const void *queries, int k, int nprobe, const void *dist, const void *labels, const lb_cancel *ctx)
{
    return knn_args(p, nq, queries, k, dist, labels, ctx, [&]() -> int {
        if (nprobe > 0) return LB_OK;
        p->set_error("nprobe=%d: at least one list is probed", nprobe);
        return LB_ERR_INVALID_ARG;
    });
}

} // namespace

extern "C" {

lb_gpu_ivf *lb_gpu_ivf_new(int device, int dim, int metric, int order, int nlist, const float *centroids, int *out_status)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    if (dim <= 0 || metric < 0 || metric > 2 || order < 0 || order > 1 || nlist <= 0 || !centroids) { st(LB_ERR_INVALID_ARG); return nullptr; }
    if (dim > LB_MAX_DIM || nlist > IVF_MAX_NLIST) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    int inner = LB_OK;
    lb_gpu_ivf *h = handle_open<lb_gpu_ivf>(device, out_status, [&](lb_gpu_ivf *p) {
        p->dims = dim;
        p->metric = metric;
        p->order = order;
        p->nlist = nlist;
        p->h_cent.assign(centroids, centroids + (size_t)nlist * dim);
        p->h_sizes.assign((size_t)nlist, 0);
        p->h_vsizes.assign((size_t)nlist, 0);
        for (int i = 0; i < 2; i++) {
            p->d_off[i].alloc((size_t)nlist + 1);
            LB_HIP(hipMemset(p->d_off[i].get(), 0, ((size_t)nlist + 1) * 4));
            p->d_voff[i].alloc((size_t)nlist + 1);
            LB_HIP(hipMemset(p->d_voff[i].get(), 0, ((size_t)nlist + 1) * 4));
        }
        p->coarse = lb_gpu_index_new(device, dim, metric, &inner);
        if (!p->coarse) return;
        inner = lb_gpu_index_set_order(p->coarse, order);
        if (inner == LB_OK) inner = lb_gpu_index_add(p->coarse, nlist, centroids, nullptr);
        LB_HIP(hipSetDevice(device));
    });
    if (h && inner != LB_OK) { // the centroids did not get onto the device
        handle_free(h);
        st(inner);
        return nullptr;
    }
    return h;
}

void lb_gpu_ivf_free(lb_gpu_ivf *p) { handle_free(p); }
const char *lb_gpu_ivf_last_error(const lb_gpu_ivf *p) { return handle_last_error(p); }
int lb_gpu_ivf_dim(const lb_gpu_ivf *p) { return p ? p->dims : 0; }
int lb_gpu_ivf_metric(const lb_gpu_ivf *p) { return p ? p->metric : 0; }
int lb_gpu_ivf_order(const lb_gpu_ivf *p) { return p ? p->order : 0; }
int lb_gpu_ivf_nlist(const lb_gpu_ivf *p) { return p ? p->nlist : 0; }
int64_t lb_gpu_ivf_ntotal(const lb_gpu_ivf *p) { return handle_ntotal(p); }

int64_t lb_gpu_ivf_hbm_bytes(const lb_gpu_ivf *p)
{
    if (!p) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_ivf *>(p)->mu);
    const RowFilter &f = p->filter;
    return (int64_t)(p->d_rows.count() * 4 + p->d_ids.count() * 8 + (p->d_assign.count() + p->d_list[0].count() + p->d_list[1].count()) * 4 +
                     (p->d_off[0].count() + p->d_off[1].count()) * 4 +
                     (p->d_voff[0].count() + p->d_voff[1].count() + p->d_vlist[0].count() + p->d_vlist[1].count()) * 4 +
                     f.mask.count() + (f.rowmap.count() + f.scratch.count()) * 4) + lb_gpu_index_hbm_bytes(p->coarse);
}

int lb_gpu_ivf_get_centroids(lb_gpu_ivf *p, float *out)
{
    if (!p || !out) return LB_ERR_INVALID_ARG;
    std::copy(p->h_cent.begin(), p->h_cent.end(), out); // (fixed at creation)
    return LB_OK;
}

int lb_gpu_ivf_reserve(lb_gpu_ivf *p, int64_t n_total)
{
    return handle_reserve(p, n_total, [](lb_gpu_ivf *h, int64_t need) { ivf_grow(h, need, h->has_ids); });
}

// ---- the row filter (lb_handle.h) ---------------------------------------------------------------------------------------
int64_t lb_gpu_ivf_nvisible(const lb_gpu_ivf *p) { return filter_nvisible(p); }
int lb_gpu_ivf_set_filter(lb_gpu_ivf *p, const uint8_t *mask, int64_t n)
{
    Lease vis;
    return filter_set(p, mask, n, visible_builder(p, vis));
}
int lb_gpu_ivf_filter_int64(lb_gpu_ivf *p, const int64_t *column, int64_t n, int64_t value, int op, const uint8_t *validity,
                            int64_t validity_offset, int combine)
{
    Lease vis;
    return filter_column<int64_t>(p, column, n, value, op, validity, validity_offset, combine, visible_builder(p, vis));
}
int lb_gpu_ivf_filter_float32(lb_gpu_ivf *p, const float *column, int64_t n, float value, int op, const uint8_t *validity,
                              int64_t validity_offset, int combine)
{
    Lease vis;
    return filter_column<float>(p, column, n, value, op, validity, validity_offset, combine, visible_builder(p, vis));
}

int lb_gpu_ivf_add(lb_gpu_ivf *p, int64_t n, const float *vectors, const int64_t *ids) { return add_impl(p, n, vectors, ids, false); }
int lb_gpu_ivf_add_device(lb_gpu_ivf *p, int64_t n, const float *d_vectors, const int64_t *d_ids) { return add_impl(p, n, d_vectors, d_ids, true); }

int lb_gpu_ivf_list_sizes(lb_gpu_ivf *p, int64_t *sizes)
{
    if (!p || !sizes) return LB_ERR_INVALID_ARG;
    std::shared_lock<std::shared_mutex> g(p->mu);
    std::copy(p->h_sizes.begin(), p->h_sizes.end(), sizes);
    return LB_OK;
}

int lb_gpu_ivf_assignments(lb_gpu_ivf *p, int64_t row0, int64_t n, int32_t *lists)
{
    if (!p || row0 < 0 || n < 0 || (n > 0 && !lists)) return LB_ERR_INVALID_ARG;
    if (n == 0) return LB_OK;
    std::shared_lock<std::shared_mutex> g(p->mu);
    if (const int st = rows_in_range(p, row0, n)) return st;
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        LB_HIP(hipMemcpy(lists, p->d_assign.get() + row0, (size_t)n * 4, hipMemcpyDeviceToHost)); // (list numbers are below 2^16)
        return LB_OK;
    });
}

int lb_gpu_ivf_search_device_ctx(lb_gpu_ivf *p, int64_t nq, const float *d_queries, int k, int nprobe, float *d_dist, int64_t *d_labels,
                                 void *stream, const lb_cancel *ctx)
{
    const int rc = search_args(p, nq, d_queries, k, nprobe, d_dist, d_labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    std::shared_lock<std::shared_mutex> g(p->mu);
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    Lease sc;
    return guard(p, s, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        return ivf_search_dev(p, nq, d_queries, k, nprobe, d_dist, d_labels, s, ctx, sc);
    });
}

int lb_gpu_ivf_search_ctx(lb_gpu_ivf *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels, const lb_cancel *ctx)
{
    const int rc = search_args(p, nq, queries, k, nprobe, dist, labels, ctx);
    if (rc != LB_OK || nq == 0) return rc;
    return host_knn(
        p, nq, (size_t)p->dims * 4, k, dist, labels,
        [&](Lease &dq, Lease &, hipStream_t s) { LB_HIP(hipMemcpyAsync(dq.p, queries, (size_t)nq * p->dims * 4, hipMemcpyHostToDevice, s)); },
        [&](Lease &dq, float *d_dist, int64_t *d_labels, hipStream_t s, Lease &sc) {
            return ivf_search_dev(p, nq, dq.as<float>(), k, nprobe, d_dist, d_labels, s, ctx, sc);
        });
}

int lb_gpu_ivf_search(lb_gpu_ivf *p, int64_t nq, const float *queries, int k, int nprobe, float *dist, int64_t *labels)
{
    return lb_gpu_ivf_search_ctx(p, nq, queries, k, nprobe, dist, labels, nullptr);
}

int lb_gpu_ivf_last_search_stats(lb_gpu_ivf *p, int64_t out[4])
{
    if (!p || !out) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->err_mu);
    std::copy(p->stats, p->stats + 4, out);
    return LB_OK;
}

int lb_gpu_ivf_set_profiling(lb_gpu_ivf *p, int enable)
{
    if (!p) return LB_ERR_INVALID_ARG;
    p->profiling.store(enable != 0);
    return LB_OK;
}

int lb_gpu_ivf_last_timing(lb_gpu_ivf *p, float ms[4])
{
    if (!p || !ms) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->err_mu);
    std::copy(p->timing, p->timing + 4, ms);
    return LB_OK;
}

int lb_gpu_ivf_last_build_timing(lb_gpu_ivf *p, float *ms)
{
    if (!p || !ms) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(p->err_mu);
    *ms = p->build_ms;
    return LB_OK;
}

} // extern "C"
