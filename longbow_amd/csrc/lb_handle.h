// lb_handle.h -- the host shell of every handle behind the C ABI: the flat index (lb_gpu_index: index.hip, index_search.hip,
// simd_api.hip, through lb_index.h), the code-index handles (lb_gpu_pq, lb_gpu_bq, lb_gpu_sq8) and the IVF handles (lb_gpu_ivf,
// lb_gpu_ivfpq; what those two share beyond this is in lb_ivf_host.h).  HandleCore, the error functions, guard() and HostSlab
// serve all of them and the handle-less calls of simd_api.hip (guard_device); CodeHandle and what follows it serve the code and
// IVF handles.  Header-only, nothing exported.
//
// The rules every entry point keeps:
//   * nothing but an lb_status leaves the library: the body of an entry point runs inside guard() or guard_device();
//   * a pooled buffer (Lease) that a stream-enqueuing body uses is declared OUTSIDE the guard and the stream is passed to it: an
//     error drains the stream before the buffer goes back to the pool, where a concurrent call could lease it;
//   * searches and reads take `mu` shared; adds, reserve and whatever changes the row filter take it alone.
#pragma once
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_host.h"

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>

namespace lb {
#pragma GCC visibility push(hidden) // nothing here, the instantiations over the handles' types included, is exported

// What every handle has: its device, the reader / writer lock of its entry points and the text of its last failure.
struct HandleCore {
    int device = 0;
    std::shared_mutex mu;
    mutable std::mutex err_mu;
    std::string last_error;
    void set_error(const char *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        std::lock_guard<std::mutex> g(err_mu);
        try {
            last_error = buf;
        } catch (...) { // out of host memory: the status code still reaches the caller
        }
    }
};

// What every code-index handle has; lb_gpu_bq, lb_gpu_sq8 and lb_gpu_pq derive from it and add their own buffers.  Those are
// destroyed before `stream` (members of the derived struct go first): harmless, every *_free drains the device under the
// writer lock before it deletes the handle.
struct CodeHandle : HandleCore {
    int dims = 0;
    int64_t n = 0, capacity = 0; // rows stored, rows allocated
    Stream stream;
};

// A failed HIP call as a status and, on a handle (h is null in the handle-less calls), its text.  The failure is reported through
// the return code: HIP's per-thread last error is cleared, so that the thread's next entry point does not find it in its
// LB_LAUNCH_CHECK and report a kernel launch that never failed.
inline int hip_fail(HandleCore *h, const HipErr &e)
{
    (void)hipGetLastError();
    if (h) h->set_error("HIP error %d (%s) in %s", (int)e.e, hipGetErrorString(e.e), e.what);
    return e.e == hipErrorOutOfMemory ? LB_ERR_OOM : LB_ERR_HIP;
}

inline int ctx_fail(HandleCore *h, int st)
{
    if (h) h->set_error(st == LB_ERR_CANCELLED ? "context canceled" : "context deadline exceeded");
    return st;
}

// The shell of an entry point: nothing but an lb_status leaves the library.  `s`, where given, is the stream the body
// enqueued on (hipStreamLegacy for the null stream): it is drained before the answer, so that no kernel still runs on what the
// caller gets back or on a pooled buffer that returns.
template <class F> int guard(HandleCore *h, hipStream_t s, F &&body) noexcept
{
    try {
        return body();
    } catch (const HipErr &e) {
        if (s) (void)hipStreamSynchronize(s);
        return hip_fail(h, e);
    } catch (const CtxErr &c) { // a context polled between launches: what is already on the stream finishes first
        if (s) (void)hipStreamSynchronize(s);
        return ctx_fail(h, c.code);
    } catch (const std::bad_alloc &) {
        if (s) (void)hipStreamSynchronize(s);
        if (h) h->set_error("out of host memory");
        return LB_ERR_OOM;
    } catch (...) {
        if (s) (void)hipStreamSynchronize(s);
        if (h) h->set_error("internal error (exception)");
        return LB_ERR_INTERNAL;
    }
}
// the same for a call that has a device and no handle: the status alone
template <class F> int guard_device(hipStream_t s, F &&body) noexcept { return guard(nullptr, s, std::forward<F>(body)); }

constexpr size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// The slab of a host-pointer search of nq queries (row_bytes each) for k results: [queries | dist | labels], the same bytes in
// pinned host memory and on the device.  Small results (a few queries: the latency path) are written by the last kernel
// straight into the pinned slab (`direct`): no device-to-host copy and no second wait behind it.  Each handle stages it its
// own way (the flat index: a pooled HostStage with a stream per caller; PQ: leases on the handle's stream).
struct HostSlab {
    size_t row_bytes, qb, db, lb, doff, loff, total;
    bool direct;
    HostSlab(int64_t nq, size_t row_bytes_, int k)
        : row_bytes(row_bytes_), qb((size_t)nq * row_bytes_), db(up16((size_t)nq * k * 4)), lb((size_t)nq * k * 8), doff(up16(qb)),
          loff(doff + db), total(loff + lb), direct(db + lb <= ((size_t)64 << 10))
    {
    }
    // the requests' queries, one after the other, into the slab at hb
    void gather(HostReq *const *reqs, int nreq, char *hb) const
    {
        for (int i = 0; i < nreq; i++) {
            const size_t b = (size_t)reqs[i]->nq * row_bytes;
            std::memcpy(hb, reqs[i]->q, b);
            hb += b;
        }
    }
    // every request's rows of the result out of the slab at hb
    void scatter(HostReq *const *reqs, int nreq, const char *hb, int k) const
    {
        size_t row = 0;
        for (int i = 0; i < nreq; i++) {
            const size_t n = (size_t)reqs[i]->nq * k;
            std::memcpy(reqs[i]->dist, hb + doff + row * 4, n * 4);
            std::memcpy(reqs[i]->labels, hb + loff + row * 8, n * 8);
            row += n;
        }
    }
};

// lb_gpu_*_set_search_combining / _combining_stats of a handle with a `combiner` (lb_combine.h)
template <class H> int combining_set(H *h, int enable)
{
    if (!h) return LB_ERR_INVALID_ARG;
    h->combiner.on.store(enable ? 1 : 0);
    return LB_OK;
}
template <class H> int combining_stats(const H *h, int64_t out[2])
{
    if (!h || !out) return LB_ERR_INVALID_ARG;
    out[0] = h->combiner.batches.load();
    out[1] = h->combiner.requests.load();
    return LB_OK;
}

// rows per staging piece of the host-pointer codec calls: at most 64 Mi elements, so that the pooled buffers stay small
inline int64_t piece_rows(int dims) { return std::max<int64_t>(1, ((int64_t)64 << 20) / dims); }

// Consecutive 16-byte-aligned pieces of one buffer.  A layout is a function of a Carve that take()s its pieces in order and
// returns `off`; lease_layout runs it once to size the lease and once more to bind the pointers, which hold only then.
struct Carve {
    char *base;
    size_t off = 0;
    template <class T> T *take(size_t bytes)
    {
        T *p = reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(base) + off);
        off += up16(bytes);
        return p;
    }
};
template <class L> void lease_layout(Lease &sc, int device, L &&layout)
{
    sc.reset(device, layout(Carve{nullptr}));
    layout(Carve{sc.as<char>()});
}

// The capacity a code buffer of `cap` rows of `row_bytes` grows to when `need` rows are asked for: geometric, at least 4096
// rows; a buffer already beyond 1 GiB grows by at most 25 % (or to the request), so that no second copy of a large buffer is
// ever transient.  Each handle's *_grow allocates and copies its own buffers.
constexpr int64_t grow_capacity(int64_t cap, int64_t need, size_t row_bytes)
{
    if ((size_t)cap * row_bytes > ((size_t)1 << 30)) return std::max<int64_t>(need, cap + cap / 4);
    return std::max<int64_t>(std::max<int64_t>(need, cap * 2), 4096);
}
static_assert(grow_capacity(0, 1, 8) == 4096, "first allocation");
static_assert(grow_capacity(4096, 4097, 8) == 8192, "doubling");
static_assert(grow_capacity(4096, 100000, 8) == 100000, "a request beyond the double");
static_assert(grow_capacity((int64_t)1 << 27, ((int64_t)1 << 27) + 1, 8) == (int64_t)1 << 28, "exactly 1 GiB held still doubles");
static_assert(grow_capacity(((int64_t)1 << 27) + 4, ((int64_t)1 << 27) + 5, 8) == 167772165, "beyond 1 GiB held: + 25 %");
static_assert(grow_capacity(((int64_t)1 << 27) + 4, (int64_t)1 << 29, 8) == (int64_t)1 << 29, "beyond 1 GiB held: the request");

// ---- refusals ---------------------------------------------------------------------------------------------------------
// BQ and SQ8: a selection key holds the row in 32 bits and the counts are u32.  PQ holds up to 2^32 - 1 rows without a row
// filter and this many with one (the filter's list and the counts of its compaction are u32)
constexpr int64_t kMaxRows = 0x7fffffffll;

inline int rows_fit(CodeHandle *h, int64_t have, int64_t more)
{
    if (more <= kMaxRows - have) return LB_OK;
    h->set_error("2^31 or more codes per handle");
    return LB_ERR_UNSUPPORTED;
}

// rows [row0, row0 + n) of the stored ones; the caller holds `mu`
inline int rows_in_range(CodeHandle *h, int64_t row0, int64_t n)
{
    if (n <= h->n && row0 <= h->n - n) return LB_OK;
    h->set_error("rows [%lld, %lld) outside the %lld stored codes", (long long)row0, (long long)(row0 + n), (long long)h->n);
    return LB_ERR_INVALID_ARG;
}

// INVALID_ARG, then whatever `ready` refuses (SQ8: an untrained handle), then UNSUPPORTED, then the context: what a k-NN
// entry point answers before it touches the device
template <class Ready>
int knn_args(HandleCore *h, int64_t nq, const void *queries, int k, const void *dist, const void *labels, const lb_cancel *ctx, Ready &&ready)
{
    if (!h || nq < 0 || k <= 0 || (nq > 0 && (!queries || !dist || !labels))) return LB_ERR_INVALID_ARG;
    if (const int st = ready()) return st;
    if (k > LB_MAX_K) { h->set_error("k=%d exceeds the supported maximum %d", k, LB_MAX_K); return LB_ERR_UNSUPPORTED; }
    if (const int st = ctx_state(ctx)) return ctx_fail(h, st);
    return LB_OK;
}
inline int knn_args(HandleCore *h, int64_t nq, const void *queries, int k, const void *dist, const void *labels, const lb_cancel *ctx)
{
    return knn_args(h, nq, queries, k, dist, labels, ctx, [] { return (int)LB_OK; });
}

// ---- construction and the simple entry points -------------------------------------------------------------------------
// The device drained under the writer lock, then own(p), what a handle must give back by hand before its members go (the flat
// index's pools and corpus buffer), then the handle.
template <class T, class Own> void handle_free(T *p, Own &&own)
{
    if (!p) return;
    {
        std::unique_lock<std::shared_mutex> g(p->mu);
        (void)hipSetDevice(p->device);
        (void)hipDeviceSynchronize();
        own(p);
    }
    delete p;
}
template <class T> void handle_free(T *p) { handle_free(p, [](T *) {}); }

// A handle on `device` with its stream; init(p) fills the index's own fields with the device current and may throw.
// *out_status (nullable) says why nullptr comes back.
template <class T, class Init> T *handle_open(int device, int *out_status, Init &&init)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    if (!device_ok(device)) { st(LB_ERR_NO_DEVICE); return nullptr; }
    auto *p = new (std::nothrow) T();
    if (!p) { st(LB_ERR_OOM); return nullptr; }
    p->device = device;
    try {
        LB_HIP(hipSetDevice(device));
        LB_HIP(hipStreamCreateWithFlags(&p->stream.h, hipStreamNonBlocking));
        init(p);
    } catch (const HipErr &e) {
        st(e.e == hipErrorOutOfMemory ? LB_ERR_OOM : LB_ERR_HIP);
        handle_free(p);
        return nullptr;
    } catch (...) {
        st(LB_ERR_INTERNAL);
        handle_free(p);
        return nullptr;
    }
    st(LB_OK);
    return p;
}

// BQ and SQ8: a handle of 1..LB_MAX_DIM dimensions
template <class T, class Init> T *handle_new(int device, int dims, int *out_status, Init &&init)
{
    if (dims <= 0 || dims > LB_MAX_DIM) {
        if (out_status) *out_status = dims <= 0 ? LB_ERR_INVALID_ARG : LB_ERR_UNSUPPORTED;
        return nullptr;
    }
    return handle_open<T>(device, out_status, [&](T *p) {
        p->dims = dims;
        init(p);
    });
}

inline const char *handle_last_error(const HandleCore *h)
{
    if (!h) return "null handle";
    std::lock_guard<std::mutex> g(h->err_mu);
    return h->last_error.c_str();
}

inline int64_t handle_ntotal(const CodeHandle *h)
{
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<CodeHandle *>(h)->mu); // (adds commit under the writer lock)
    return h->n;
}

// BQ and SQ8: room for n_total rows, by the index's own grow(p, n_total)
template <class T, class Grow> int handle_reserve(T *p, int64_t n_total, Grow &&grow)
{
    if (!p || n_total < 0) return LB_ERR_INVALID_ARG;
    if (const int st = rows_fit(p, 0, n_total)) return st;
    std::unique_lock<std::shared_mutex> g(p->mu);
    return guard(p, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(p->device));
        grow(p, n_total);
        return LB_OK;
    });
}

// ---- the row filter of a code handle ------------------------------------------------------------------------------------
// A byte per row (visible iff non-zero) and, built from it, the ascending list of the visible rows.  There is one form: with a
// filter a search walks the n_visible positions of the list, whatever share of the rows it holds; the keys of the selection
// carry positions, which order as rows do, and the finish maps them back (BQ, SQ8; the PQ handle's list kernels put the rows
// themselves into their entries).  The buffers are allocated by the first filter; while
// `on` they hold room for `capacity` rows (the handle's *_grow keeps them in step through grow) and mask[0, n) are the stored
// rows' bytes.  They are the handle's own, not pooled: they outlive every call.
// A handle that can forget rows (lb_ivf_host.h) sets `live` once a row is removed: a byte per row, zero for a removed one.  The
// mask is then the EFFECTIVE mask, the caller's filter AND live: a filter call ANDs `live` into what it has written before the
// list is built, and clearing the filter leaves mask = live in force.  For every other handle it stays null and changes nothing.
struct RowView {
    const uint32_t *rowmap; // nullptr: rows [0, n) as they are
    int64_t n;              // rows (positions) to search
};

struct RowFilter {
    DevBuf<uint8_t> mask;     // [capacity]
    DevBuf<uint32_t> rowmap;  // [capacity]; [0, n_visible) hold
    DevBuf<uint32_t> scratch; // [compact_scratch_words(capacity)]: launch_compact_mask's
    int64_t n_visible = 0;
    bool on = false;
    const uint8_t *live = nullptr; // [capacity], the handle's; null: no row has been removed

    RowView view(int64_t n) const { return on ? RowView{rowmap.get(), n_visible} : RowView{nullptr, n}; }

    // room for `cap` rows; an active filter's bytes of the n stored rows and its list are kept; all or nothing
    void reserve(int64_t n, int64_t cap)
    {
        if (mask.count() >= (size_t)cap) return;
        DevBuf<uint8_t> nm;
        DevBuf<uint32_t> nr, ns;
        nm.alloc((size_t)cap);
        nr.alloc((size_t)cap);
        ns.alloc((size_t)compact_scratch_words(cap));
        if (on && n > 0) {
            LB_HIP(hipMemcpy(nm.get(), mask.get(), (size_t)n, hipMemcpyDeviceToDevice));
            LB_HIP(hipMemcpy(nr.get(), rowmap.get(), (size_t)n_visible * 4, hipMemcpyDeviceToDevice));
        }
        mask = std::move(nm);
        rowmap = std::move(nr);
        scratch = std::move(ns);
    }
    // the handle's *_grow: an active filter's buffers stay in step with the codes'
    void grow(int64_t n, int64_t cap) { if (on) reserve(n, cap); }
    // the list and n_visible from mask[0, n); drains s
    void rebuild(int64_t n, hipStream_t s)
    {
        uint32_t total = 0;
        if (n > 0) {
            launch_compact_mask(mask.get(), n, rowmap.get(), scratch.get(), s);
            LB_LAUNCH_CHECK();
            LB_HIP(hipMemcpyAsync(&total, scratch.get() + (compact_scratch_words(n) - 1), 4, hipMemcpyDeviceToHost, s));
            LB_HIP(hipStreamSynchronize(s));
        }
        n_visible = (int64_t)total;
    }
    // rows [n_old, n_new) are stored (room for them reserved) and about to be committed: they are visible
    void on_append(int64_t n_old, int64_t n_new, hipStream_t s)
    {
        if (!on) return;
        LB_HIP(hipMemsetAsync(mask.get() + n_old, 1, (size_t)(n_new - n_old), s));
        rebuild(n_new, s);
    }
};

struct FilteredHandle : CodeHandle {
    RowFilter filter;
};

inline int64_t filter_nvisible(const FilteredHandle *h)
{
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<FilteredHandle *>(h)->mu);
    return h->filter.view(h->n).n;
}

// A row filter covers at most kMaxRows rows: what a filter call answers on a larger handle, and an add that would take a
// filtered handle beyond it, before the device is touched (only the PQ handle can hold that many)
inline int filter_fits(CodeHandle *h, int64_t rows)
{
    if (rows <= kMaxRows) return LB_OK;
    h->set_error("a row filter covers fewer than 2^31 rows, the handle would hold %lld", (long long)rows);
    return LB_ERR_UNSUPPORTED;
}

// What a handle derives from the filter beyond the list (the IVF handle's visible lists): built(s) runs after rebuild and before
// the filter is on, enqueues on s, and throws like any body of guard(); the code handles have nothing to build.
struct NothingToBuild {
    void operator()(hipStream_t) const {}
};

// lb_gpu_*_set_filter: n bytes of the host, or nullptr to clear
template <class Built = NothingToBuild> int filter_set(FilteredHandle *h, const uint8_t *mask, int64_t n, Built &&built = Built())
{
    if (!h) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    RowFilter &f = h->filter;
    if (!mask && !f.live) { f.on = false; return LB_OK; }
    if (mask && n != h->n) {
        h->set_error("filter mask has %lld bytes, the handle holds %lld rows", (long long)n, (long long)h->n);
        return LB_ERR_INVALID_ARG;
    }
    if (const int st = filter_fits(h, h->n)) return st;
    return guard(h, h->stream, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        f.reserve(h->n, h->capacity);
        f.on = false; // a failure from here on leaves the handle without a filter, not with half of one
        if (!mask) { // removed rows stay hidden: the live rows are what is visible
            n = h->n;
            if (n > 0) LB_HIP(hipMemcpyAsync(f.mask.get(), f.live, (size_t)n, hipMemcpyDeviceToDevice, h->stream));
        } else if (n > 0) {
            LB_HIP(hipMemcpy(f.mask.get(), mask, (size_t)n, hipMemcpyHostToDevice));
            if (f.live) launch_and_bytes(f.mask.get(), f.live, n, h->stream);
        }
        f.rebuild(n, h->stream);
        built(h->stream);
        f.on = true;
        return LB_OK;
    });
}

// lb_gpu_*_filter_int64 / _float32: the predicate evaluated on the device into the mask (launch_match_*)
template <class T, class Built = NothingToBuild>
int filter_column(FilteredHandle *h, const T *column, int64_t n, T value, int op, const uint8_t *validity, int64_t voff, int combine,
                  Built &&built = Built())
{
    if (!h || op < 0 || op > 5 || voff < 0) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    RowFilter &f = h->filter;
    if (n != h->n || (n > 0 && !column)) {
        h->set_error("filter column has %lld values, the handle holds %lld rows", (long long)n, (long long)h->n);
        return LB_ERR_INVALID_ARG;
    }
    if (const int st = filter_fits(h, h->n)) return st;
    Lease dcol, dval;
    return guard(h, h->stream, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        hipStream_t s = h->stream;
        const int comb = combine && f.on ? 1 : 0; // AND into "no filter" replaces
        f.reserve(h->n, h->capacity);
        f.on = false; // as filter_set
        if (n > 0) {
            dcol.reset(h->device, (size_t)n * sizeof(T));
            LB_HIP(hipMemcpyAsync(dcol.p, column, (size_t)n * sizeof(T), hipMemcpyHostToDevice, s));
            const uint8_t *d_val = nullptr;
            if (validity) {
                const size_t vb = (size_t)((voff + n + 7) / 8);
                dval.reset(h->device, vb);
                LB_HIP(hipMemcpyAsync(dval.p, validity, vb, hipMemcpyHostToDevice, s));
                d_val = dval.as<uint8_t>();
            }
            if constexpr (sizeof(T) == 8) launch_match_int64(dcol.as<int64_t>(), n, (int64_t)value, op, d_val, voff, f.mask.get(), comb, s);
            else launch_match_float32(dcol.as<float>(), n, (float)value, op, d_val, voff, f.mask.get(), comb, s);
            if (f.live && !comb) launch_and_bytes(f.mask.get(), f.live, n, s); // (a mask that is ANDed into holds `live` already)
        }
        f.rebuild(n, s);
        built(s);
        f.on = true;
        return LB_OK;
    });
}

// ---- k-NN of host queries -----------------------------------------------------------------------------------------------
// Host queries -> pooled device buffers -> search -> results back, on the handle's stream under the reader lock; the caller
// has answered knn_args and nq == 0.  put(dq, stage, s) enqueues what leaves the nq queries in dq (code_bytes each) as the
// device codes the index searches, `stage` being a lease for whatever it stages; search(dq, d_dist, d_labels, s, scratch) is
// the index's k-NN of device codes and returns its status with the stream drained.
template <class Put, class Search>
int host_knn(CodeHandle *h, int64_t nq, size_t code_bytes, int k, float *dist, int64_t *labels, Put &&put, Search &&search)
{
    std::shared_lock<std::shared_mutex> g(h->mu);
    Lease dq, dout, stage, scratch;
    return guard(h, h->stream, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        hipStream_t s = h->stream;
        const size_t db = up16((size_t)nq * k * 4), lb = (size_t)nq * k * 8;
        dq.reset(h->device, (size_t)nq * code_bytes);
        dout.reset(h->device, db + lb);
        put(dq, stage, s);
        float *d_dist = dout.as<float>();
        int64_t *d_labels = reinterpret_cast<int64_t *>(dout.as<char>() + db);
        const int rc = search(dq, d_dist, d_labels, s, scratch);
        if (rc != LB_OK) return rc;
        LB_HIP(hipMemcpy(dist, d_dist, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
        LB_HIP(hipMemcpy(labels, d_labels, lb, hipMemcpyDeviceToHost));
        return LB_OK;
    });
}

// ---- codec calls on host rows -------------------------------------------------------------------------------------------
// n host rows of in_row bytes -> n host rows of out_row bytes, in pieces of piece_rows through two pooled buffers;
// run(d_in, d_out, cnt) is the index's device-pointer form of the call: it returns its status with its stream drained.
template <class Run> int host_codec(CodeHandle *h, int64_t n, const void *in, size_t in_row, void *out, size_t out_row, Run &&run)
{
    Lease din, dout;
    return guard(h, h->stream, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        const int64_t piece = std::min(n, piece_rows(h->dims));
        din.reset(h->device, (size_t)piece * in_row);
        dout.reset(h->device, (size_t)piece * out_row);
        for (int64_t r0 = 0; r0 < n; r0 += piece) {
            const int64_t cnt = std::min(piece, n - r0);
            LB_HIP(hipMemcpy(din.p, static_cast<const char *>(in) + (size_t)r0 * in_row, (size_t)cnt * in_row, hipMemcpyHostToDevice));
            if (const int rc = run(din.p, dout.p, cnt)) return rc;
            LB_HIP(hipMemcpy(static_cast<char *>(out) + (size_t)r0 * out_row, dout.p, (size_t)cnt * out_row, hipMemcpyDeviceToHost));
        }
        return LB_OK;
    });
}

#pragma GCC visibility pop
} // namespace lb
