// index.hip -- host side of liblongbow_gpu.so: the C ABI of include/longbow_gpu.h.
//
// Mirrors the contract of Longbow's gpu.Index (internal/gpu/interface.go:3-19) as
// the FAISS binding realises it (internal/gpu/faiss_gpu.go:44-167): opaque handle,
// int return codes, Add appends, Search is safe from many threads at once
// (RWMutex: Add/Close exclusive, Search shared), nothing aborts the process.
//
// There is NO CPU fallback in this library: without a HIP device every entry point
// returns LB_ERR_NO_DEVICE / NULL.
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_host.h"
#include "lb_index.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace lb;

std::atomic<int> g_vmm_fail_next{0}; // test hook: the next mapping attempt reports a driver refusal

namespace {

constexpr size_t kStageBytes = 32u << 20; // pinned staging slab (x2)
// Add batches of at least this many bytes pin the caller's buffer instead of staging it (0 = never)
std::atomic<long long> g_add_register_min{(long long)lb_tunable("LB_ADD_REGISTER_MIN_MB", 64) << 20};

} // namespace

void drop_f16_image(lb_gpu_index *h)
{
    h->d_Xh.reset();
    h->d_norm2c.reset();
    h->xh_rows = h->xh_cap = 0;
    h->xh_centred = h->xh_c_ok = h->xh_offset_dom = false;
    h->xh_rho = 0.f;
    h->xh_exact = false;
    if (h->d_xh_rho2) (void)hipMemset(h->d_xh_rho2.get(), 0, sizeof(uint32_t));
}

void drop_split_image(lb_gpu_index *h)
{
    h->d_Xs.reset();
    h->xs_rows = 0;
}

// Make room for `need` rows.  The corpus itself grows in place (VmmBuf); only the small per-row side
// arrays (norms, ids, mask, liveness: 18 B per row) are reallocated geometrically and copied.  Without VMM the
// corpus follows the same malloc + copy scheme (needs old + new resident at once).
static int grow(lb_gpu_index *h, int64_t need)
{
    const size_t row_bytes = (size_t)h->dim * h->elem_bytes();
    int64_t cap = std::max<int64_t>(need, h->capacity * 2);
    cap = std::max<int64_t>(cap, 1024);
    if (h->vmm.ok) {
        try {
            h->vmm.ensure((size_t)need * row_bytes);
            h->d_X = reinterpret_cast<float *>(h->vmm.base);
            h->x_rows_cap = (int64_t)(h->vmm.mapped / row_bytes);
        } catch (const HipErr &e) {
            (void)hipGetLastError(); // do not leave a sticky error behind for the caller's next HIP call
            if (e.e == hipErrorOutOfMemory) throw;
            // The driver refused to extend the mapping (hipMemSetAccess reports "invalid argument" for some
            // chunk sequences on this stack, tools/probe/): move the rows into one hipMalloc'd buffer and
            // grow geometrically from here on.
            DevBuf<char> nx;
            nx.alloc((size_t)cap * row_bytes);
            if (h->n > 0) {
                hipError_t ce = hipMemcpyAsync(nx.get(), h->d_X, (size_t)h->n * row_bytes, hipMemcpyDeviceToDevice, h->add_stream);
                if (ce == hipSuccess) ce = hipStreamSynchronize(h->add_stream);
                if (ce != hipSuccess) throw HipErr{ce, "hipMemcpyAsync (leaving the mapped corpus)"};
            }
            h->vmm.destroy();
            h->d_X = reinterpret_cast<float *>(nx.release());
            h->x_rows_cap = cap;
        }
    }
    if (need <= h->capacity && (h->vmm.ok || need <= h->x_rows_cap)) return LB_OK;
    if (need <= h->capacity) cap = h->capacity; // only the corpus buffer (malloc mode) is short
    // the new arrays stay locals until every copy has succeeded: a throw on the way frees them and leaves the handle as it was
    DevBuf<char> nx;
    DevBuf<float> n2, rn;
    DevBuf<int64_t> ni;
    DevBuf<uint8_t> nm, nl;
    const bool grow_x = !h->vmm.ok && cap > h->x_rows_cap;
    const bool grow_side = cap > h->capacity;
    if (grow_x) nx.alloc((size_t)cap * row_bytes);
    if (grow_side) {
        n2.alloc((size_t)cap);
        rn.alloc((size_t)cap);
        ni.alloc((size_t)cap);
        nm.alloc((size_t)cap);
        nl.alloc(((size_t)cap + 3) & ~(size_t)3); // (whole words: launch_remove_rows)
    }
    if (h->n > 0) {
        if (nx) LB_HIP(hipMemcpyAsync(nx.get(), h->d_X, (size_t)h->n * row_bytes, hipMemcpyDeviceToDevice, h->add_stream));
        if (grow_side) {
            LB_HIP(hipMemcpyAsync(n2.get(), h->d_norm2.get(), (size_t)h->n * sizeof(float), hipMemcpyDeviceToDevice, h->add_stream));
            LB_HIP(hipMemcpyAsync(rn.get(), h->d_rnorm.get(), (size_t)h->n * sizeof(float), hipMemcpyDeviceToDevice, h->add_stream));
            LB_HIP(hipMemcpyAsync(ni.get(), h->d_ids.get(), (size_t)h->n * sizeof(int64_t), hipMemcpyDeviceToDevice, h->add_stream));
            LB_HIP(hipMemcpyAsync(nm.get(), h->d_mask.get(), (size_t)h->n, hipMemcpyDeviceToDevice, h->add_stream));
            LB_HIP(hipMemcpyAsync(nl.get(), h->d_live.get(), (size_t)h->n, hipMemcpyDeviceToDevice, h->add_stream));
        }
        LB_HIP(hipStreamSynchronize(h->add_stream));
    }
    if (nx) {
        if (h->d_X) (void)hipFree(h->d_X);
        h->d_X = reinterpret_cast<float *>(nx.release());
        h->x_rows_cap = cap;
    }
    if (grow_side) {
        h->d_norm2 = std::move(n2);
        h->d_rnorm = std::move(rn);
        h->d_ids = std::move(ni);
        h->d_mask = std::move(nm);
        h->d_live = std::move(nl);
        h->capacity = cap;
    }
    drop_split_image(h); // the mirror is rebuilt at the new capacity by the next sync_split_image
    if (h->d_Xh) drop_f16_image(h); // its planes are `capacity` rows apart: rebuilt by the next sync_f16_image
    return LB_OK;
}

// grow(), giving the accelerator copies back first when the device is full.  The fp16 copy (half the corpus's bytes again)
// and the split-bf16 image (all of them again) only speed searches up; the rows are the index.  An Add / reserve that runs
// out of memory while either is resident frees them and tries once more before it reports LB_ERR_OOM; the copy is then
// taken again only when twice the usual margin is free (sync_f16_image), so an index at the edge does not rebuild it per Add.
static int grow_or_shed(lb_gpu_index *h, int64_t need)
{
    try {
        return grow(h, need);
    } catch (const HipErr &e) {
        if (e.e != hipErrorOutOfMemory || (!h->d_Xh && !h->d_Xs)) throw;
        (void)hipGetLastError();
        if (h->d_Xh) {
            drop_f16_image(h);
            h->xh_shed = true;
        }
        if (h->d_Xs) { // (the explicit split-image mode cannot be kept: back to the default routes)
            drop_split_image(h);
            h->cand_mode.store(LB_CAND_AUTO);
        }
        buf_pool().trim(h->device);
        return grow(h, need);
    }
}

// Recompute the visible-row list from d_mask (caller holds the exclusive lock).  The list is used
// by searches when at most LB_ROWMAP_MAX_PCT % of the corpus is visible (default 95; measured on
// 1.25M x 1536: time scales with the visible fraction all the way up -- 8.6 ms unfiltered, 7.8 ms at
// 90 %, 4.5 ms at 50 %, 1.16 ms at 10 % for 256 queries -- so only near-total masks keep the per-row test).
void rebuild_rowmap(lb_gpu_index *h)
{
    h->smap_valid = false; // the corpus view changes (callers hold the exclusive lock)
    h->rowmap_on = false;
    h->n_visible = h->n;
    if (!h->has_mask || h->n == 0) return;
    static const int max_pct = lb_tunable("LB_ROWMAP_MAX_PCT", 95);
    if (max_pct <= 0) return;
    hipStream_t s = h->add_stream;
    if (h->d_rowmap.count() < (size_t)h->n) h->d_rowmap.alloc((size_t)h->capacity);
    const int64_t words = compact_scratch_words(h->n);
    if (h->d_cscratch.count() < (size_t)words) h->d_cscratch.alloc((size_t)compact_scratch_words(h->capacity));
    launch_compact_mask(h->d_mask.get(), h->n, h->d_rowmap.get(), h->d_cscratch.get(), s);
    uint32_t total = 0;
    LB_HIP(hipMemcpyAsync(&total, h->d_cscratch.get() + (words - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    h->n_visible = (int64_t)total;
    h->rowmap_on = h->n_visible * 100 <= h->n * (int64_t)max_pct;
}

static __global__ void iota_ids_kernel(int64_t *ids, int64_t start, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[start + i] = start + i;
}

// what the norm statistics (d_maxnorm2's two words: max ||x||^2 and the smallest non-zero ||x||^2, as float bits) say of the rows
void set_norm_flags(lb_gpu_index *h, const uint32_t nbits[2])
{
    const uint32_t maxbits = nbits[0]; // >= +inf <=> a row with an inf or NaN component
    h->nonfinite = maxbits >= 0x7f800000u;
    // fp16 single-product candidates: no element may overflow fp16 (|x_i| <= ||x|| <= 2^13) and the smallest non-zero
    // row norm bounds the subnormal rounding term of the contraction's error bound (>= 2^-6: kernels_gemm_tall16.hip)
    const float mx = __builtin_bit_cast(float, maxbits), mn = __builtin_bit_cast(float, nbits[1]);
    h->f16_ok = !h->nonfinite && mx <= 67108864.0f /* 2^26 */ && (nbits[1] == 0x7f800000u || mn >= 0.000244140625f /* 2^-12 */);
    h->norm_spread = !h->nonfinite && nbits[1] != 0x7f800000u && mx > 256.0f * mn;
}

// Rows [h->n, h->n + n) are already in d_X; finish the append (norms, ids, mask, liveness).
static void finish_add(lb_gpu_index *h, int64_t n, const int64_t *ids_src, bool ids_on_device)
{
    hipStream_t s = h->add_stream;
    const int64_t start = h->n;
    if (h->i8_rows)
        launch_row_norms_i8(h->rows_i8() + (size_t)start * h->dim, n, h->dim, h->norm2_i8() + start, s);
    else
        with_rows(h, [&](auto X) {
            launch_row_norms(X + (size_t)start * h->dim, n, h->dim, h->d_norm2.get() + start, h->d_rnorm.get() + start, h->d_maxnorm2.get(), s);
        });
    if (ids_src) {
        if (!h->has_ids && start > 0)
            hipLaunchKernelGGL(iota_ids_kernel, dim3((unsigned)((start + 255) / 256)), dim3(256), 0, s, h->d_ids.get(),
                               (int64_t)0, start);
        LB_HIP(hipMemcpyAsync(h->d_ids.get() + start, ids_src, (size_t)n * sizeof(int64_t),
                              ids_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        h->has_ids = true;
    } else if (h->has_ids) {
        hipLaunchKernelGGL(iota_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->d_ids.get(), start, n);
    }
    LB_HIP(hipMemsetAsync(h->d_mask.get() + start, 1, (size_t)n, s));
    LB_HIP(hipMemsetAsync(h->d_live.get() + start, 0xff, (size_t)n, s)); // appended rows are live
    uint32_t nbits[2] = {0, 0};
    LB_HIP(hipMemcpyAsync(nbits, h->d_maxnorm2.get(), sizeof nbits, hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    LB_LAUNCH_CHECK();
    set_norm_flags(h, nbits);
    h->n += n; // the rows are committed from here on: nothing below may fail the call (a retry would duplicate them)
    try {
        sync_split_image(h);
    } catch (const HipErr &) { // no room for the bf16 mirror: back to the default routes
        (void)hipGetLastError();
        h->cand_mode.store(LB_CAND_AUTO);
        drop_split_image(h);
    }
    sync_f16_image(h); // (never throws: without the image the route stages f32 rows)
    try {
        rebuild_rowmap(h); // appended rows are visible; keep the list in step with the corpus
    } catch (const HipErr &) { // searches fall back to the per-row mask test
        (void)hipGetLastError();
        h->rowmap_on = false;
        h->n_visible = h->n;
    }
}

// bring the split-bf16 mirror up to date with d_X (no-op unless the mode is enabled)
void sync_split_image(lb_gpu_index *h)
{
    if (h->cand_mode.load() != 1 || h->dim % 32 != 0 || h->n == 0 || h->f16_rows || h->i8_rows) return;
    if (!h->d_Xs || h->xs_rows > h->n) {
        drop_split_image(h);
        h->d_Xs.alloc((size_t)h->capacity * h->dim);
    }
    if (h->xs_rows < h->n) {
        launch_split_bf16(h->d_X + (size_t)h->xs_rows * h->dim, h->d_Xs.get() + (size_t)h->xs_rows * h->dim,
                          h->n - h->xs_rows, h->dim, h->add_stream);
        LB_HIP(hipStreamSynchronize(h->add_stream));
        h->xs_rows = h->n;
    }
}

// Bring the corpus's fp16 image up to date (caller holds the exclusive lock), or drop it when it is not wanted any more.
// Wanted: the fp16 route is on offer for this index (mode, dimension, norms, size) and the copy fits -- half the corpus's
// bytes again, taken only while that leaves max(2 GiB, 1/16 of the device) free.  Never fails the caller: without the image
// the route stages the f32 rows.
void sync_f16_image(lb_gpu_index *h)
{
    const int cm = h->cand_mode.load();
    // (from 16,384 rows -- the size from which a sampled threshold exists.  Round 4 brought it down from 262,144, to 65,536 first:
    // 100k x 768 at 256 queries 0.298 -> 0.163 ms, 1024: 0.82 -> 0.43; 200k x 768: 0.49 -> 0.21, 1.25 -> 0.57; +50 % of a corpus
    // of this size is 0.15-0.4 GB)
    static const int64_t f16_image_min_rows = lb_tunable("LB_F16_IMAGE_MIN_ROWS", 16384);
    const bool l2 = h->metric == LB_METRIC_EUCLIDEAN;
    // (L2: the image is centred, so what must fit fp16 are the centred norms -- known once the centre is)
    const bool range_ok = l2 ? (!h->nonfinite && (h->xh_declined_n == 0 || h->n >= 2 * h->xh_declined_n)) : h->f16_ok;
    // (an int8 index has no image: its searches read the int8 rows)
    const bool want = h->xh_mode.load() != 0 && !h->xh_failed && !h->i8_rows && range_ok && h->n > 0 &&
                      (cm == LB_CAND_F16 || (cm == LB_CAND_AUTO && h->n >= f16_image_min_rows));
    try {
        if (!want || (h->d_Xh && (h->xh_cap < h->n || h->xh_rows > h->n))) {
            drop_f16_image(h);
            if (!want) return;
        }
        hipStream_t s = h->add_stream;
        if (!h->d_Xh) {
            const int pd = corpus_f16_plane_dims();
            const size_t need = (size_t)h->capacity * (size_t)((h->dim + pd - 1) / pd * pd) * 2 // (whole planes, the last zero-padded)
                                + (l2 ? (size_t)h->capacity * sizeof(float) : 0);
            size_t fr = 0, tot = 0;
            LB_HIP(hipMemGetInfo(&fr, &tot));
            const size_t keep = std::max<size_t>((size_t)2 << 30, tot / 16) * (h->xh_shed ? 2 : 1);
            if (fr < need + keep) return; // (not remembered: memory may be free again at the next Add)
            h->d_Xh.alloc(need - (l2 ? (size_t)h->capacity * sizeof(float) : 0)); // (refused: not tried again, below)
            h->xh_cap = h->capacity;
            h->xh_rows = 0;
            if (l2) { // the centre: column means of the rows there are (fixed from here on: appended rows are shifted by the same)
                const int dpad = ((h->dim + 31) & ~31) + 8;
                h->d_center.ensure((size_t)dpad);
                h->d_cstats.ensure(2);
                h->d_norm2c.alloc((size_t)h->capacity);
                const uint32_t init[2] = {0u, 0x7f800000u};
                LB_HIP(hipMemcpyAsync(h->d_cstats.get(), init, sizeof init, hipMemcpyHostToDevice, s));
                Lease part(h->device, (size_t)256 * h->dim * sizeof(float));
                with_rows(h, [&](auto X) { launch_column_means(X, h->n, h->dim, part.as<float>(), h->d_center.get(), dpad, s); });
                LB_HIP(hipStreamSynchronize(s)); // (the lease goes back to the pool)
                h->xh_centred = true;
            }
        }
        if (h->xh_rows < h->n) {
            const float *center = h->xh_centred ? h->d_center.get() : nullptr;
            // (fp16 rows: a relayout of the rows, or their centred form)
            with_rows(h, [&](auto X) { launch_corpus_to_f16(X, h->xh_rows, h->n, h->dim, h->d_Xh.get(), h->xh_cap, s, center); });
            if (h->xh_centred) {
                with_rows(h, [&](auto X) {
                    launch_row_norms(X + (size_t)h->xh_rows * h->dim, h->n - h->xh_rows, h->dim, h->d_norm2c.get() + h->xh_rows, nullptr,
                                     h->d_cstats.get(), s, center);
                });
                uint32_t cb[2] = {0, 0};
                LB_HIP(hipMemcpyAsync(cb, h->d_cstats.get(), sizeof cb, hipMemcpyDeviceToHost, s));
                LB_HIP(hipStreamSynchronize(s));
                const float mx = __builtin_bit_cast(float, cb[0]), mn = __builtin_bit_cast(float, cb[1]);
                h->xh_c_ok = cb[0] < 0x7f800000u && mx <= 67108864.0f /* 2^26 */ && (cb[1] == 0x7f800000u || mn >= 0.000244140625f /* 2^-12 */);
                if (!h->xh_c_ok) { // the spread itself is beyond fp16: no image for this index until it has doubled
                    h->xh_declined_n = h->n;
                    drop_f16_image(h);
                    return;
                }
                std::vector<float> hc((size_t)h->dim);
                LB_HIP(hipMemcpy(hc.data(), h->d_center.get(), hc.size() * sizeof(float), hipMemcpyDeviceToHost));
                double c2 = 0.0;
                for (float v : hc) c2 += (double)v * (double)v;
                h->xh_offset_dom = c2 > 4.0 * (double)mx;
            }
            { // the loss of the new rows' images, measured (the candidate keys' error bound: key_bound)
                if (!h->d_xh_rho2) {
                    h->d_xh_rho2.alloc(1);
                    LB_HIP(hipMemsetAsync(h->d_xh_rho2.get(), 0, sizeof(uint32_t), s));
                }
                with_rows(h, [&](auto X) { launch_f16_residual(X, h->xh_rows, h->n, h->dim, center, h->d_xh_rho2.get(), s); });
                uint32_t rb = 0;
                LB_HIP(hipMemcpyAsync(&rb, h->d_xh_rho2.get(), sizeof rb, hipMemcpyDeviceToHost, s));
                LB_HIP(hipStreamSynchronize(s));
                const float r2 = __builtin_bit_cast(float, rb);
                // (a ratio beyond the worst case of normal fp16 values, 2^-22, means elements in the subnormal range or flushed
                // to zero carry weight: still a valid bound as long as it is finite and small enough to be of use)
                h->xh_rho = (rb < 0x7f800000u && r2 <= 1.0e-4f) ? std::sqrt(r2) * 1.000001f : 0.f;
                h->xh_exact = h->f16_rows && !h->xh_centred && rb == 0; // (the image is the rows: rho_x = 0)
            }
            LB_HIP(hipStreamSynchronize(s));
            h->xh_rows = h->n;
        }
    } catch (const HipErr &) {
        (void)hipGetLastError();
        drop_f16_image(h);
        h->xh_failed = true;
    }
}

template <typename T>
static int filter_column(lb_gpu_index *h, const T *column, int64_t n, T value, int op, const uint8_t *validity,
                         int64_t voff, int combine)
{
    if (!h || op < 0 || op > 5 || voff < 0) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    if (n != h->n || (n > 0 && !column)) {
        h->set_error("filter column has %lld values, index has %lld rows", (long long)n, (long long)h->n);
        return LB_ERR_INVALID_ARG;
    }
    if (n == 0) { h->has_mask = h->has_filter = true; h->rowmap_on = false; return LB_OK; }
    Lease dcol, dval; // column (and validity bitmap) go up through pooled buffers on the index's own stream
    return guard(h, h->add_stream, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        dcol.reset(h->device, (size_t)n * sizeof(T));
        T *d_col = dcol.as<T>();
        uint8_t *d_val = nullptr;
        LB_HIP(hipMemcpyAsync(d_col, column, (size_t)n * sizeof(T), hipMemcpyHostToDevice, h->add_stream));
        if (validity) {
            const size_t vb = (size_t)((voff + n + 7) / 8);
            dval.reset(h->device, vb);
            d_val = dval.as<uint8_t>();
            LB_HIP(hipMemcpyAsync(d_val, validity, vb, hipMemcpyHostToDevice, h->add_stream));
        }
        const int comb = (combine && h->has_mask) ? 1 : 0; // AND into "no filter" == replace
        if constexpr (sizeof(T) == 8)
            launch_match_int64(reinterpret_cast<const int64_t *>(d_col), n, (int64_t)value, op, d_val, voff, h->d_mask.get(), comb, h->add_stream);
        else
            launch_match_float32(reinterpret_cast<const float *>(d_col), n, (float)value, op, d_val, voff, h->d_mask.get(), comb, h->add_stream);
        // (a replaced mask knows nothing of the removed rows; one that was ANDed into held them as zeros already)
        if (!comb && h->n_dead > 0) launch_and_bytes(h->d_mask.get(), h->d_live.get(), n, h->add_stream);
        LB_LAUNCH_CHECK();
        LB_HIP(hipStreamSynchronize(h->add_stream));
        h->has_mask = h->has_filter = true;
        rebuild_rowmap(h);
        return LB_OK;
    });
}

int dtype_mismatch(lb_gpu_index *h, int call)
{
    if (h->dtype() == call) return LB_OK;
    static const char *const what[3] = {"this index holds float32 rows: use the float32 entry point",
                                        "this index holds float16 rows: use the _f16 entry point",
                                        "this index holds int8 rows: use the _i8 entry point"};
    h->set_error("%s", what[h->dtype()]);
    return LB_ERR_INVALID_ARG;
}


// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int lb_gpu_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

const char *lb_gpu_version(void) { return "longbow_gpu 0.1.0 (gfx950, HIP)"; }

const char *lb_gpu_status_string(int status)
{
    switch (status) {
    case LB_OK: return "ok";
    case LB_ERR_INVALID_ARG: return "invalid argument";
    case LB_ERR_CLOSED: return "index is closed";
    case LB_ERR_NO_DEVICE: return "GPU not available";
    case LB_ERR_HIP: return "HIP runtime error";
    case LB_ERR_OOM: return "out of device memory";
    case LB_ERR_UNSUPPORTED: return "unsupported configuration";
    case LB_ERR_CANCELLED: return "context canceled";
    case LB_ERR_DEADLINE: return "context deadline exceeded";
    default: return "internal error";
    }
}

// dtype: 0 float32, 1 float16, 2 int8 (simd.DataType)
static lb_gpu_index *index_new(int device, int dim, int metric, int *out_status, int dtype)
{
    auto st = [&](int v) { if (out_status) *out_status = v; };
    if (dim <= 0 || metric < 0 || metric > 2) { st(LB_ERR_INVALID_ARG); return nullptr; }
    // the kernels stage one query row (and the re-rank a 256 x 64-float tile plus up to 4096 keys) in LDS:
    // LB_MAX_DIM keeps every launch inside the 160 KB a workgroup may declare
    if (dim > LB_MAX_DIM) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    if (dtype == 2) {
        // int8: the reference registers no cosine kernel (DispatchDistance: "no kernel found"); its dot chains are exact
        // integers only while floor(D / 4) + D mod 4 <= 1024 (kernels_i8.hip)
        if (metric == LB_METRIC_COSINE) { st(LB_ERR_UNSUPPORTED); return nullptr; }
        if (metric == LB_METRIC_DOT && dim / 4 + dim % 4 > 1024) { st(LB_ERR_UNSUPPORTED); return nullptr; }
    }
    if (!device_ok(device)) { st(LB_ERR_NO_DEVICE); return nullptr; }
    auto *h = new (std::nothrow) lb_gpu_index();
    if (!h) { st(LB_ERR_OOM); return nullptr; }
    h->device = device; h->dim = dim; h->metric = metric;
    h->f16_rows = dtype == 1;
    h->i8_rows = dtype == 2;
    // (fp16 rows: UNROLL4 is the only order of the reference's F16 functions, internal/simd/simd.go:767-848; int8 rows: the
    // order is accepted and changes nothing, the int8 arithmetic has one form)
    if (h->f16_rows || h->i8_rows) h->order.store(LB_ORDER_UNROLL4);
    const int rc = guard(h, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(device));
        LB_HIP(hipStreamCreateWithFlags(&h->add_stream.h, hipStreamNonBlocking));
        h->d_maxnorm2.alloc(2);
        const uint32_t norm_init[2] = {0u, 0x7f800000u}; // max ||x||^2 so far, smallest non-zero ||x||^2 so far (float bits)
        LB_HIP(hipMemcpy(h->d_maxnorm2.get(), norm_init, sizeof norm_init, hipMemcpyHostToDevice));
        static const int use_vmm = lb_tunable("LB_VMM", 1);
        if (use_vmm) (void)h->vmm.init(device); // on failure: geometric hipMalloc + copy
        return LB_OK;
    });
    st(rc);
    if (rc == LB_OK) return h;
    lb_gpu_index_free(h);
    return nullptr;
}

lb_gpu_index *lb_gpu_index_new(int device, int dim, int metric, int *out_status)
{
    return index_new(device, dim, metric, out_status, 0);
}
lb_gpu_index *lb_gpu_index_new_f16(int device, int dim, int metric, int *out_status)
{
    return index_new(device, dim, metric, out_status, 1);
}
lb_gpu_index *lb_gpu_index_new_i8(int device, int dim, int metric, int *out_status)
{
    return index_new(device, dim, metric, out_status, 2);
}
int lb_gpu_index_dtype(const lb_gpu_index *h) { return h ? h->dtype() : 0; }

int64_t lb_gpu_index_hbm_bytes(const lb_gpu_index *h)
{
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_index *>(h)->mu);
    const int pd = corpus_f16_plane_dims();
    int64_t b = h->vmm.ok ? (int64_t)h->vmm.mapped : h->x_rows_cap * (int64_t)h->dim * (int64_t)h->elem_bytes();
    b += h->capacity * (int64_t)(2 * sizeof(float) + sizeof(int64_t) + 2); // norms, inverse norms, ids, mask, liveness
    if (h->d_rowmap) b += (int64_t)h->d_rowmap.count() * (int64_t)sizeof(uint32_t);
    if (h->d_Xs) b += h->capacity * (int64_t)h->dim * (int64_t)sizeof(float);
    if (h->d_Xh) b += h->xh_cap * (int64_t)((h->dim + pd - 1) / pd * pd) * 2;
    if (h->d_norm2c) b += h->xh_cap * (int64_t)sizeof(float);
    return b;
}

void lb_gpu_index_free(lb_gpu_index *h)
{
    // the device drained under the writer lock, then what is the flat index's own: the two pools and the corpus buffer; every
    // other buffer, the streams and the events go with their members
    handle_free(h, [](lb_gpu_index *h) {
        {
            std::lock_guard<std::mutex> g2(h->ws_mu);
            h->ws_free.clear();
            h->hs_free.clear();
        }
        if (h->vmm.ok) h->vmm.destroy();
        else if (h->d_X) (void)hipFree(h->d_X);
        h->d_X = nullptr;
    });
}

const char *lb_gpu_last_error(const lb_gpu_index *h) { return handle_last_error(h); }

int lb_gpu_index_set_order(lb_gpu_index *h, int order)
{
    if (!h || (order != LB_ORDER_SEQ && order != LB_ORDER_UNROLL4)) return LB_ERR_INVALID_ARG;
    h->order.store(order);
    return LB_OK;
}

int lb_gpu_index_set_candidate_mode(lb_gpu_index *h, int mode)
{
    if (!h || mode < LB_CAND_F32_MFMA || mode > LB_CAND_F16) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    if (h->f16_rows && mode != LB_CAND_AUTO && mode != LB_CAND_F16) {
        h->set_error("candidate mode %d needs f32 rows; an fp16 index takes AUTO or F16", mode);
        return LB_ERR_UNSUPPORTED;
    }
    if (h->i8_rows && mode != LB_CAND_AUTO) {
        h->set_error("candidate mode %d needs f32 rows; an int8 index takes AUTO only", mode);
        return LB_ERR_UNSUPPORTED;
    }
    if ((mode == LB_CAND_SPLIT_BF16 || mode == LB_CAND_SPLIT_BF16_INREG) && h->dim % 32 != 0) {
        h->set_error("split-bf16 candidates need dim %% 32 == 0 (dim = %d)", h->dim);
        return LB_ERR_UNSUPPORTED;
    }
    const int rc = guard(h, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        h->cand_mode.store(mode);
        if (mode == 1) sync_split_image(h);
        else drop_split_image(h);
        sync_f16_image(h);
        return LB_OK;
    });
    if (rc != LB_OK) h->cand_mode.store(LB_CAND_AUTO);
    return rc;
}

int lb_gpu_index_set_f16_image(lb_gpu_index *h, int mode)
{
    if (!h || mode < 0 || mode > 1) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    return guard(h, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        h->xh_mode.store(mode);
        if (mode) { h->xh_failed = h->xh_shed = false; h->xh_declined_n = 0; }
        sync_f16_image(h);
        return LB_OK;
    });
}

int64_t lb_gpu_index_f16_image_bytes(const lb_gpu_index *h)
{
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_index *>(h)->mu); // (the copy is built and dropped under the writer lock)
    const int pd = corpus_f16_plane_dims();
    return h->d_Xh.get() ? (int64_t)h->xh_cap * ((h->dim + pd - 1) / pd * pd) * 2 : 0;
}

int64_t lb_gpu_index_ntotal(const lb_gpu_index *h)
{
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_index *>(h)->mu); // (Add commits its rows under the writer lock)
    return h->n;
}
int64_t lb_gpu_index_nvisible(const lb_gpu_index *h)
{
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> g(const_cast<lb_gpu_index *>(h)->mu);
    return h->has_mask ? h->n_visible : h->n; // (rebuild_rowmap's count: every filter call, removal and add brings it up to date)
}
int lb_gpu_index_dim(const lb_gpu_index *h) { return h ? h->dim : 0; }
int lb_gpu_index_device(const lb_gpu_index *h) { return h ? h->device : -1; }

int lb_gpu_index_reserve(lb_gpu_index *h, int64_t n_total)
{
    if (!h || n_total < 0) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    return guard(h, nullptr, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        return grow_or_shed(h, n_total);
    });
}

static int add_host(lb_gpu_index *h, int64_t n, const void *vectors, const int64_t *ids, int dtype)
{
    if (!h || n < 0 || (n > 0 && !vectors)) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    if (const int rc = dtype_mismatch(h, dtype)) return rc;
    if (n == 0) return LB_OK;
    if (h->n + n > (int64_t)0xffffffffll) { h->set_error("more than 2^32 rows per device"); return LB_ERR_UNSUPPORTED; }
    return guard(h, h->add_stream, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        grow_or_shed(h, h->n + n);
        for (int i = 0; i < 2; i++) {
            h->h_stage[i].ensure(kStageBytes);
            if (!h->stage_ev[i]) LB_HIP(hipEventCreateWithFlags(&h->stage_ev[i].h, hipEventDisableTiming));
        }
        const size_t total = (size_t)n * h->dim * h->elem_bytes();
        const char *src = reinterpret_cast<const char *>(vectors);
        char *dst = reinterpret_cast<char *>(h->d_X) + (size_t)h->n * h->dim * h->elem_bytes();
        size_t off = 0;
        // Large batches: pin the caller's buffer (the Arrow values buffer) for the duration of the call and
        // DMA straight out of it -- no host-side copy (SURVEY 8b ownership row: "the shim hipHostRegisters
        // the Arrow values buffer for the duration of the call").  Small batches, or a buffer the driver
        // will not pin, go through the double-buffered pinned slabs below.
        if (total >= (size_t)g_add_register_min.load() && g_add_register_min.load() > 0) {
            void *reg = const_cast<void *>(vectors);
            if (hipHostRegister(reg, total, hipHostRegisterDefault) == hipSuccess) {
                hipError_t e = hipSuccess;
                const size_t piece = (size_t)256 << 20;
                for (size_t o = 0; o < total && e == hipSuccess; o += piece)
                    e = hipMemcpyAsync(dst + o, src + o, std::min(piece, total - o), hipMemcpyHostToDevice, h->add_stream);
                if (e == hipSuccess) e = hipStreamSynchronize(h->add_stream);
                (void)hipHostUnregister(reg);
                if (e != hipSuccess) throw HipErr{e, "hipMemcpyAsync (registered add)"};
                off = total;
            } else {
                (void)hipGetLastError();
            }
        }
        // host buffer -> pinned slab (memcpy) -> HBM (async DMA), two slabs in flight
        int slab = 0;
        bool used[2] = {false, false};
        while (off < total) {
            const size_t len = std::min(kStageBytes, total - off);
            if (used[slab]) LB_HIP(hipEventSynchronize(h->stage_ev[slab]));
            std::memcpy(h->h_stage[slab].get(), src + off, len);
            LB_HIP(hipMemcpyAsync(dst + off, h->h_stage[slab].get(), len, hipMemcpyHostToDevice, h->add_stream));
            LB_HIP(hipEventRecord(h->stage_ev[slab], h->add_stream));
            used[slab] = true;
            slab ^= 1;
            off += len;
        }
        finish_add(h, n, ids, false);
        return LB_OK;
    });
}

int lb_gpu_index_add(lb_gpu_index *h, int64_t n, const float *vectors, const int64_t *ids)
{
    return add_host(h, n, vectors, ids, 0);
}
int lb_gpu_index_add_f16(lb_gpu_index *h, int64_t n, const uint16_t *vectors, const int64_t *ids)
{
    return add_host(h, n, vectors, ids, 1);
}
int lb_gpu_index_add_i8(lb_gpu_index *h, int64_t n, const int8_t *vectors, const int64_t *ids)
{
    return add_host(h, n, vectors, ids, 2);
}

static int add_device(lb_gpu_index *h, int64_t n, const void *d_vectors, const int64_t *d_ids, int dtype)
{
    if (!h || n < 0 || (n > 0 && !d_vectors)) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    if (const int rc = dtype_mismatch(h, dtype)) return rc;
    if (n == 0) return LB_OK;
    if (h->n + n > (int64_t)0xffffffffll) { h->set_error("more than 2^32 rows per device"); return LB_ERR_UNSUPPORTED; }
    return guard(h, h->add_stream, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        grow_or_shed(h, h->n + n);
        LB_HIP(hipMemcpyAsync(reinterpret_cast<char *>(h->d_X) + (size_t)h->n * h->dim * h->elem_bytes(), d_vectors,
                              (size_t)n * h->dim * h->elem_bytes(), hipMemcpyDeviceToDevice, h->add_stream));
        finish_add(h, n, d_ids, true);
        return LB_OK;
    });
}

int lb_gpu_index_add_device(lb_gpu_index *h, int64_t n, const float *d_vectors, const int64_t *d_ids)
{
    return add_device(h, n, d_vectors, d_ids, 0);
}
int lb_gpu_index_add_f16_device(lb_gpu_index *h, int64_t n, const uint16_t *d_vectors, const int64_t *d_ids)
{
    return add_device(h, n, d_vectors, d_ids, 1);
}
int lb_gpu_index_add_i8_device(lb_gpu_index *h, int64_t n, const int8_t *d_vectors, const int64_t *d_ids)
{
    return add_device(h, n, d_vectors, d_ids, 2);
}

int lb_gpu_index_set_filter(lb_gpu_index *h, const uint8_t *mask, int64_t n)
{
    if (!h) return LB_ERR_INVALID_ARG;
    std::unique_lock<std::shared_mutex> g(h->mu);
    if (!mask && h->n_dead == 0) { h->has_mask = h->has_filter = false; h->rowmap_on = false; h->smap_valid = false; return LB_OK; }
    if (!mask) { // removed rows stay hidden: the view is the live rows (d_mask holds a cleared filter's bytes: recomposed)
        return guard(h, h->add_stream, [&]() -> int {
            LB_HIP(hipSetDevice(h->device));
            LB_HIP(hipMemcpyAsync(h->d_mask.get(), h->d_live.get(), (size_t)h->n, hipMemcpyDeviceToDevice, h->add_stream));
            h->has_filter = false;
            h->has_mask = true;
            rebuild_rowmap(h);
            return LB_OK;
        });
    }
    if (n != h->n) { h->set_error("filter mask has %lld bytes, index has %lld rows", (long long)n, (long long)h->n); return LB_ERR_INVALID_ARG; }
    return guard(h, h->add_stream, [&]() -> int {
        LB_HIP(hipSetDevice(h->device));
        if (n > 0) LB_HIP(hipMemcpy(h->d_mask.get(), mask, (size_t)n, hipMemcpyHostToDevice));
        if (h->n_dead > 0) { // the effective mask: the caller's bytes AND live
            launch_and_bytes(h->d_mask.get(), h->d_live.get(), n, h->add_stream);
            LB_LAUNCH_CHECK();
        }
        h->has_mask = h->has_filter = true;
        rebuild_rowmap(h);
        return LB_OK;
    });
}

int lb_gpu_index_filter_int64(lb_gpu_index *h, const int64_t *column, int64_t n, int64_t value, int op,
                              const uint8_t *validity, int64_t validity_offset, int combine)
{
    return filter_column<int64_t>(h, column, n, value, op, validity, validity_offset, combine);
}

int lb_gpu_index_filter_float32(lb_gpu_index *h, const float *column, int64_t n, float value, int op,
                                const uint8_t *validity, int64_t validity_offset, int combine)
{
    return filter_column<float>(h, column, n, value, op, validity, validity_offset, combine);
}

#ifdef LB_DIAG
void lb_debug_vmm_fail_next(int v) { g_vmm_fail_next.store(v); } // the next in-place growth is refused (-> hipMalloc + copy)
void lb_debug_set_add_register_min(long long bytes) { g_add_register_min.store(bytes); } // ingest A/B (tools/bench_add.py)
#endif

} // extern "C"
