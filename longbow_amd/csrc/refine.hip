// refine.hip -- lb_gpu_index_refine* (include/longbow_gpu.h): the batched exact refine of shortlists on the rows of a float32 or
// float16 index.  Per batch of queries three launches: the shortlists become ascending lists of distinct valid rows
// (launch_refine_prepare), every list position gets its key (launch_refine_scan; before it the query norms of a cosine index),
// and the selection of the IVF handles takes the k smallest keys of each query (launch_ivf_select: an IvfBatch without probe
// slots reads seg[q][0] as the query's count, which is the list's length).  The bodies run inside guard() (lb_handle.h).
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_host.h"
#include "lb_index.h"
#include "lb_ivf.h"
#include "lb_refine.h"

#include <algorithm>
#include <cstring>

using namespace lb;

namespace {

constexpr int64_t kRefineBatch = 1024;                // queries per batch at most: the scan's grid takes them along y
constexpr int64_t kRefineScratch = (int64_t)1 << 28;  // bytes of lists and keys a batch may hold
constexpr int64_t kRefineHostPiece = (int64_t)64 << 20; // bytes of queries, shortlists and results a host-pointer piece may stage
constexpr size_t kRefinePinnedBytes = (size_t)1 << 20;  // a host-pointer call that moves at most this much stages through pinned memory
static_assert(LB_REFINE_MAX_C <= IVF_SELECT_LDS_KEYS, "a query's keys fit the selection's LDS copy");

// what every form answers before it touches the device; LB_OK with nq == 0 means "nothing to do"
int refine_args(lb_gpu_index *h, int64_t nq, const void *queries, int64_t c, const void *rows, int k, int order, const void *dist,
                const void *labels, const lb_cancel *ctx)
{
    if (!h || nq < 0 || (order != -1 && order != LB_ORDER_SEQ && order != LB_ORDER_UNROLL4) || c < 1 || c > LB_REFINE_MAX_C || k <= 0)
        return LB_ERR_INVALID_ARG;
    if (k > LB_MAX_K) { h->set_error("k=%d exceeds the supported maximum %d", k, LB_MAX_K); return LB_ERR_UNSUPPORTED; }
    if (nq == 0) return LB_OK;
    if (!queries || !rows || !dist || !labels) return LB_ERR_INVALID_ARG;
    if (h->i8_rows) { // (fixed for the handle's life: no lock)
        h->set_error("refine reads float32 or float16 rows: not available on an int8 index");
        return LB_ERR_UNSUPPORTED;
    }
    if (const int st = ctx_state(ctx)) return ctx_fail(h, st);
    return LB_OK;
}

} // namespace

extern "C" {

int lb_gpu_index_refine_device_ctx(lb_gpu_index *h, int64_t nq, const float *d_queries, int64_t c, const int64_t *d_rows, int k,
                                   int order, float *d_dist, int64_t *d_labels, void *stream, const lb_cancel *ctx)
{
    const int arc = refine_args(h, nq, d_queries, c, d_rows, k, order, d_dist, d_labels, ctx);
    if (arc != LB_OK || nq == 0) return arc;
    std::shared_lock<std::shared_mutex> g(h->mu);
    // a private stream per call when the caller gave none (the null stream would serialise callers)
    hipStream_t s = (hipStream_t)stream;
    std::unique_ptr<Workspace> w;
    if (!s) {
        const int rc = guard(h, nullptr, [&]() -> int {
            LB_HIP(hipSetDevice(h->device));
            int kc; uint32_t cap;
            cand_geometry(1, kc, cap);
            w = acquire_ws(h, 1, cap);
            return LB_OK;
        });
        if (rc != LB_OK) return rc;
        s = w->stream;
    }
    Lease sc;
    const int rc = guard(h, s, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        if (h->n == 0) { // all padding, without a scan launch
            launch_fill_empty(d_dist, d_labels, nq * k, s);
            LB_LAUNCH_CHECK();
            LB_HIP(hipStreamSynchronize(s));
            return LB_OK;
        }
        const int ord = order == -1 ? h->order.load() : order;
        const int64_t nb = std::min(std::min(nq, kRefineBatch), std::max<int64_t>(1, kRefineScratch / (12 * c)));
        RefineBatch a{};
        a.X = h->d_X;
        a.D = h->dim;
        a.ntotal = h->n;
        a.live = h->n_dead > 0 ? h->d_live.get() : nullptr; // a removed position joins the padding
        a.c = (int)c;
        float *d_qna = nullptr;
        lease_layout(sc, h->device, [&](Carve cv) {
            a.list = cv.take<uint32_t>((size_t)nb * c * 4);
            a.len = cv.take<uint32_t>((size_t)nb * 4);
            a.qna = d_qna = cv.take<float>((size_t)nb * 4);
            a.keys = cv.take<uint64_t>((size_t)nb * c * 8);
            return cv.off;
        });
        IvfBatch sel{}; // the selection's view of a batch: no probe slots, seg[q][0] = len[q], c keys per query
        sel.np = 0;
        sel.seg = a.len;
        sel.keys = a.keys;
        sel.pmax = c;
        // a profiled call (lb_gpu_index_set_profiling) times its three steps by events, at the cost of a drain per batch
        const bool prof = h->profiling.load() != 0;
        EventH ev[4];
        float tms[3] = {0.f, 0.f, 0.f};
        if (prof)
            for (EventH &e : ev) LB_HIP(hipEventCreate(&e.h));
        auto mark = [&](int i) { if (prof) LB_HIP(hipEventRecord(ev[i], s)); };
        for (int64_t q0 = 0; q0 < nq; q0 += nb) {
            a.nq = sel.nq = (int)std::min(nb, nq - q0);
            a.Q = d_queries + (size_t)q0 * h->dim;
            a.rows = d_rows + (size_t)q0 * c;
            ctx_check(ctx);
            mark(0);
            launch_refine_prepare(a, s);
            mark(1);
            if (h->metric == LB_METRIC_COSINE) {
                ctx_check(ctx);
                launch_query_norms(ord, a.Q, nullptr, a.nq, h->dim, d_qna, s);
            }
            ctx_check(ctx);
            launch_refine_scan(h->metric, ord, h->f16_rows, a, s);
            mark(2);
            ctx_check(ctx);
            launch_ivf_select(sel, k, h->has_ids ? h->d_ids.get() : nullptr, d_dist + (size_t)q0 * k, d_labels + (size_t)q0 * k, s);
            mark(3);
            if (prof) {
                LB_HIP(hipEventSynchronize(ev[3]));
                for (int i = 0; i < 3; i++) {
                    float ms = 0.f;
                    LB_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
                    tms[i] += ms;
                }
            }
        }
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(s));
        if (prof) {
            std::lock_guard<std::mutex> pg(h->prof_mu);
            std::copy(tms, tms + 3, h->refine_ms);
        }
        return LB_OK;
    });
    if (w && rc == LB_OK) release_ws(h, std::move(w)); // (after an error the workspace is freed, not pooled)
    return rc;
}

int lb_gpu_index_refine_ctx(lb_gpu_index *h, int64_t nq, const float *queries, int64_t c, const int64_t *rows, int k, int order,
                            float *dist, int64_t *labels, const lb_cancel *ctx)
{
    const int arc = refine_args(h, nq, queries, c, rows, k, order, dist, labels, ctx);
    if (arc != LB_OK || nq == 0) return arc;
    // in pieces of queries, so that the pooled staging buffers stay small whatever nq is
    const size_t qrow = (size_t)h->dim * 4, rrow = (size_t)c * 8;
    const int64_t piece = std::min(nq, std::max<int64_t>(1, kRefineHostPiece / (int64_t)(qrow + rrow + (size_t)k * 12)));
    Lease hin, din, dout, hout;
    return guard(h, hipStreamLegacy, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        // A small call (the latency path) goes [queries | shortlists] up through one pinned block and one copy and
        // [dist | labels] back through another, as the re-rank does: two copies in place of four.  A large one copies straight
        // from and to the caller's memory: the pass through the pinned blocks costs more there than the two copies it saves
        // (measured at 1M x 768: 0.105 -> 0.080 ms at 1 x 100, 0.87 -> 1.10 ms at 1024 x 1000).
        const size_t qb = up16((size_t)piece * qrow), db = up16((size_t)piece * k * 4);
        const size_t inb = qb + (size_t)piece * rrow, outb = db + (size_t)piece * k * 8;
        const bool pinned = inb + outb <= kRefinePinnedBytes;
        din.reset(h->device, inb);
        dout.reset(h->device, outb);
        if (pinned) {
            hin.reset(h->device, inb, true);
            hout.reset(h->device, outb, true);
        }
        float *d_q = din.as<float>();
        int64_t *d_r = reinterpret_cast<int64_t *>(din.as<char>() + qb);
        float *d_d = dout.as<float>();
        int64_t *d_l = reinterpret_cast<int64_t *>(dout.as<char>() + db);
        for (int64_t q0 = 0; q0 < nq; q0 += piece) {
            const int64_t cnt = std::min(piece, nq - q0);
            const float *q_src = queries + (size_t)q0 * h->dim;
            const int64_t *r_src = rows + (size_t)q0 * c;
            if (pinned) {
                std::memcpy(hin.p, q_src, (size_t)cnt * qrow);
                std::memcpy(hin.as<char>() + qb, r_src, (size_t)cnt * rrow);
                LB_HIP(hipMemcpy(din.p, hin.p, qb + (size_t)cnt * rrow, hipMemcpyHostToDevice));
            } else {
                LB_HIP(hipMemcpy(d_q, q_src, (size_t)cnt * qrow, hipMemcpyHostToDevice));
                LB_HIP(hipMemcpy(d_r, r_src, (size_t)cnt * rrow, hipMemcpyHostToDevice));
            }
            if (const int rc = lb_gpu_index_refine_device_ctx(h, cnt, d_q, c, d_r, k, order, d_d, d_l, nullptr, ctx)) return rc;
            if (pinned) {
                LB_HIP(hipMemcpy(hout.p, dout.p, db + (size_t)cnt * k * 8, hipMemcpyDeviceToHost));
                std::memcpy(dist + (size_t)q0 * k, hout.p, (size_t)cnt * k * 4);
                std::memcpy(labels + (size_t)q0 * k, hout.as<char>() + db, (size_t)cnt * k * 8);
            } else {
                LB_HIP(hipMemcpy(dist + (size_t)q0 * k, d_d, (size_t)cnt * k * 4, hipMemcpyDeviceToHost));
                LB_HIP(hipMemcpy(labels + (size_t)q0 * k, d_l, (size_t)cnt * k * 8, hipMemcpyDeviceToHost));
            }
        }
        return LB_OK;
    });
}

int lb_gpu_index_refine(lb_gpu_index *h, int64_t nq, const float *queries, int64_t c, const int64_t *rows, int k, int order,
                        float *dist, int64_t *labels)
{
    return lb_gpu_index_refine_ctx(h, nq, queries, c, rows, k, order, dist, labels, nullptr);
}

int lb_gpu_index_refine_last_timing(lb_gpu_index *h, float ms[3])
{
    if (!h || !ms) return LB_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(h->prof_mu);
    std::copy(h->refine_ms, h->refine_ms + 3, ms);
    return LB_OK;
}

} // extern "C"
