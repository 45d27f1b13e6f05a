// lb_index.h -- what the translation units behind the index's C ABI share (index.hip: the handle and its storage;
// index_remove.hip: removal and compaction; index_search.hip: workspaces, routes and the search drivers; simd_api.hip: the re-rank
// entry points): the handle, the pooled
// per-search structs, the row view and the few functions that cross files.  The handle's lock, error text and the shell of its
// entry points (guard) are lb_handle.h's, as for every other handle.  Internal: nothing here is part of the ABI.
#pragma once
#include "../../include/longbow_gpu.h"
#include "lb_device.h"
#include "lb_handle.h"
#include "lb_host.h"

#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

using namespace lb;

struct LB_INTERNAL Event {
    EventH a, b;
    int cls = 0;
};

// What a search walks: all corpus rows (optionally testing the mask per row), or the compacted
// list of visible rows (rebuild_rowmap decides; build_call_view for a call that brings its own bitmap).
struct IndexRowView { // (lb::RowView is the code handles': a list or nothing)
    const uint8_t *mask;
    const uint32_t *rowmap;
    int64_t n;
};

struct LB_INTERNAL Workspace {
    int device = 0;
    Stream stream;
    int nq_cap = 0;
    uint32_t cap = 0;
    // the candidate state as the kernels take it (by value): pointers into the five buffers below, filled once (acquire_ws)
    CandState cs{};
    DevBuf<uint64_t> d_lists, d_tau;
    DevBuf<uint32_t> d_cnt, d_flags, d_stripes;
    DevBuf<float> d_qna;
    DevBuf<float> d_qs; // split-bf16 image of the query batch
    DevBuf<char> d_qh;  // fp16 image of the query batch (scaled per query) + [nq] inverse scales behind it
    DevBuf<int> d_qsel;
    DevBuf<int> d_iota;       // [nq_cap] 0,1,2,...: the slot list of "every query", filled once
    DevBuf<uint32_t> d_smap;  // [cap] sampled rows of the first pass
    DevBuf<uint32_t> d_done;  // [nq_cap] arrival tickets of the finish launch's split form (zero between launches)
    DevBuf<uint32_t> d_xcnt;  // [nq_cap] members handed in per query by that form (zero between launches)
    DevBuf<char> d_xscratch;  // its per-query result blocks (finish_scratch_bytes)
    // fused sample (kernels_gemm_narrow.hip, FUSED): [0] = ticket counter that only grows, [1 ..] = ready epochs per slot
    DevBuf<uint32_t> d_fsync;
    uint32_t fs_base = 0, fs_epoch = 0; // host mirror of the ticket counter; last epoch used
    uint32_t next_epoch() { return ++fs_epoch != 0 ? fs_epoch : (fs_epoch = 1); } // (0 = "never published")
    PinnedBuf<uint32_t> h_fail;  // epoch of a launch whose waits gave up
    PinnedBuf<uint32_t> h_flags;
    PinnedBuf<int> h_qsel;
    // an fp16 index's query batch widened to f32 (every query kernel downstream reads f32 queries)
    DevBuf<float> d_q;
    std::vector<Event> events;
    size_t ev_used = 0;
    const lb_cancel *ctx = nullptr; // the running call's cancellation context (or null)
    // the view of a call that brought its own row bitmap (build_call_view, index_search.hip; kernels_index_call.hip): the call's
    // effective mask (whole blocks of INDEX_CALL_BLOCK_ROWS bytes), its row list and the compaction scratch, grown on demand;
    // call_view says that cv holds, and every search of the call then reads cv where it would read row_view(h)
    DevBuf<uint8_t> d_cmask;
    DevBuf<uint32_t> d_crows, d_cscratch;
    PinnedBuf<uint32_t> h_ctotal; // the visible count, the four bytes the build brings back
    bool call_view = false;
    IndexRowView cv{nullptr, nullptr, 0};

    ~Workspace() { (void)hipSetDevice(device); }
};

// Device + pinned-host staging for the host-pointer search entry point, pooled per index so a
// serving loop does not pay hipMalloc/hipFree per call.
struct LB_INTERNAL HostStage {
    int device = 0;
    Stream stream;
    DevBuf<char> d_buf;    // [queries | dist | labels]
    PinnedBuf<char> h_buf; // the same bytes
    ~HostStage() { (void)hipSetDevice(device); }
};

// The corpus buffer grows IN PLACE: one virtual range the size of the device's HBM is reserved per index
// and physical chunks are mapped behind it as rows arrive (hipMemAddressReserve / hipMemCreate /
// hipMemMap).  Appending never copies the rows already resident and never needs old + new at once, so an
// index can grow to fill the 288 GB.  If the driver refuses any of the calls the index falls back to
// geometric hipMalloc + copy (vmm.ok == false).
extern std::atomic<int> g_vmm_fail_next; // test hook: the next mapping attempt reports a driver refusal (index.hip)

struct VmmBuf {
    bool ok = false;
    int device = 0;
    char *base = nullptr;
    size_t reserved = 0, mapped = 0, gran = 0;
    struct Chunk { hipMemGenericAllocationHandle_t h; size_t off, bytes; };
    std::vector<Chunk> chunks;

    bool init(int dev)
    {
        device = dev;
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = dev;
        size_t g = 0;
        if (hipMemGetAllocationGranularity(&g, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || g == 0) return false;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) return false;
        // the driver reports 4 KiB, but maps whose offsets are not 64 KiB-aligned are refused by
        // hipMemSetAccess (measured, tools/probe/vmm_probe.cpp): keep every chunk a multiple of 2 MiB
        gran = g < ((size_t)2 << 20) ? ((size_t)2 << 20) : g;
        reserved = ((total_b + gran - 1) / gran) * gran;
        void *ptr = nullptr;
        if (hipMemAddressReserve(&ptr, reserved, gran, nullptr, 0) != hipSuccess || !ptr) { (void)hipGetLastError(); return false; }
        base = static_cast<char *>(ptr);
        ok = true;
        return true;
    }
    // make [0, need) backed by memory; throws HipErr (OOM) when the device has no more to give
    void ensure(size_t need)
    {
        if (need <= mapped) return;
        if (need > reserved) throw lb::HipErr{hipErrorOutOfMemory, "corpus larger than the device"};
        if (g_vmm_fail_next.exchange(0)) throw lb::HipErr{hipErrorInvalidValue, "hipMemSetAccess (forced by the test hook)"};
        // geometric steps (at least the request, at least what is mapped already, at most 1 GiB beyond the
        // request): small indexes stay small, 288 GB take ~300 handles
        size_t want = need - mapped;
        size_t step = mapped < ((size_t)1 << 30) ? mapped : ((size_t)1 << 30);
        if (want < step) want = step;
        want = ((want + gran - 1) / gran) * gran;
        if (mapped + want > reserved) want = reserved - mapped;
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = device;
        hipMemGenericAllocationHandle_t hnd;
        hipError_t e = hipMemCreate(&hnd, want, &prop, 0);
        if (e != hipSuccess && want > ((need - mapped + gran - 1) / gran) * gran) { // retry with the exact need
            (void)hipGetLastError();
            want = ((need - mapped + gran - 1) / gran) * gran;
            e = hipMemCreate(&hnd, want, &prop, 0);
        }
        if (e != hipSuccess) throw lb::HipErr{hipErrorOutOfMemory, "hipMemCreate (corpus chunk)"};
        e = hipMemMap(base + mapped, want, 0, hnd, 0);
        if (e != hipSuccess) { (void)hipMemRelease(hnd); throw lb::HipErr{e, "hipMemMap"}; }
        hipMemAccessDesc acc{};
        acc.location.type = hipMemLocationTypeDevice;
        acc.location.id = device;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(base + mapped, want, &acc, 1);
        if (e != hipSuccess) {
            (void)hipMemUnmap(base + mapped, want);
            (void)hipMemRelease(hnd);
            throw lb::HipErr{e, "hipMemSetAccess"};
        }
        chunks.push_back({hnd, mapped, want});
        mapped += want;
    }
    void destroy()
    {
        for (auto &c : chunks) {
            (void)hipMemUnmap(base + c.off, c.bytes);
            (void)hipMemRelease(c.h);
        }
        chunks.clear();
        if (base) (void)hipMemAddressFree(base, reserved);
        base = nullptr;
        mapped = reserved = 0;
        ok = false;
    }
};

struct lb_gpu_index : HandleCore {
    int dim = 0, metric = 0;
    std::atomic<int> order{LB_ORDER_SEQ};

    // rows, row-major: f32, or IEEE binary16 on an fp16 index (f16_rows; typed float * for the f32 code -- an fp16 index's rows
    // are only ever read through rows_f16())
    float *d_X = nullptr; // vmm.base, or (vmm.ok false) a hipMalloc'd buffer this handle frees itself: lb_gpu_index_free
    bool f16_rows = false; // lb_gpu_index_new_f16: fixed for the handle's life
    bool i8_rows = false;  // lb_gpu_index_new_i8: signed int8 rows, fixed for the handle's life (searched by kernels_i8.hip only)
    VmmBuf vmm;             // backs d_X when vmm.ok (d_X == vmm.base): rows are appended in place
    int64_t x_rows_cap = 0; // rows d_X can hold (>= capacity of the side arrays when vmm.ok)
    int64_t n = 0, capacity = 0;
    DevBuf<float> d_norm2, d_rnorm;
    DevBuf<uint32_t> d_maxnorm2;
    bool nonfinite = false; // some row holds an inf / NaN: every search takes the exact scan path
    bool f16_ok = false;    // row norms within the fp16 single-product contraction's range (kernels_gemm_tall16.hip)
    bool norm_spread = false; // the longest row is more than 16 times the shortest non-zero one: dot-product searches then keep
                              // to the kernels with lower-bound keys under AUTO (plain keys leave such corpora to the exact scan)
    // AUTO backs off from the fp16 route on data whose neighbours are too close for its error bound (many queries then
    // fail the containment proof and are redone by the exact scan): searches left to skip it, and the next back-off span
    std::atomic<int> f16_skip{0}, f16_span{16};
    DevBuf<int64_t> d_ids;
    bool has_ids = false;
    // d_mask is the EFFECTIVE mask, (the caller's filter) AND live: row_view and every search read it alone.  has_filter: a
    // caller's filter is set; has_mask: there is one, or rows have been removed (n_dead > 0)
    DevBuf<uint8_t> d_mask;
    bool has_mask = false, has_filter = false;
    // removal (index_remove.hip): a byte per row, 0xff = live, 0 = removed (all ones, so that the bytewise AND with a filter keeps
    // whatever non-zero byte the caller gave); removed rows keep their positions until lb_gpu_index_compact.  No filter call
    // writes it.  Allocated in whole words: the position form clears its bytes by atomics on the words
    DevBuf<uint8_t> d_live;
    int64_t n_dead = 0;
    // ascending list of the rows the mask leaves visible (rebuilt whenever the mask or the corpus
    // changes); searches walk it instead of the corpus when the filter is selective enough
    DevBuf<uint32_t> d_rowmap, d_cscratch;
    int64_t n_visible = 0;
    bool rowmap_on = false;
    // strided sample of the current corpus view (sample_plan), built by the first batched search after
    // a change and shared by all searches with the same plan
    std::mutex smap_mu;
    DevBuf<uint32_t> d_smap;
    int64_t smap_span = 0;
    uint32_t smap_count = 0;
    bool smap_valid = false;
    // optional split-bf16 image of the corpus for the 3x-bf16 candidate contraction (same byte shape as d_X)
    std::atomic<int> cand_mode{LB_CAND_AUTO};
    DevBuf<float> d_Xs;
    int64_t xs_rows = 0; // rows of d_X already mirrored in d_Xs
    // fp16 image of the corpus for the single-product route (K-blocked [dim / 32][xh_cap][32], kernels_gemm_tall16.hip): kept
    // while that route is on offer and memory allows (sync_f16_image); half the bytes to stage per batched search
    DevBuf<char> d_Xh;
    int64_t xh_rows = 0, xh_cap = 0;
    std::atomic<int> xh_mode{1}; // lb_gpu_index_set_f16_image: 0 never, 1 when it pays and fits
    bool xh_failed = false;      // an allocation was refused: not tried again for this handle
    bool xh_shed = false;        // the copy was given back to let an Add through: retaken only with twice the margin free
    // L2 indexes keep the image CENTRED: fp16(x - c), c = the column means when the image was built.  L2 distances do not move
    // when both sides are shifted, the key |x - c|^2 - 2 (q - c).(x - c) = d^2 - |q - c|^2 orders rows as the plain key does, and
    // its errors scale with the centred norms: data with a large common offset (|c| >> spread), whose plain keys cancel, keeps
    // the matrix-core route.  d_norm2c: [xh_cap] centred norms (the keys' side input); d_cstats: their max / smallest non-zero
    // (float bits, as d_maxnorm2); xh_c_ok: those are within the fp16 contraction's range
    DevBuf<float> d_center, d_norm2c;
    DevBuf<uint32_t> d_cstats;
    bool xh_centred = false, xh_c_ok = false;
    // what the image loses, measured: max over its rows of |x - fp16(x)| / |x| (kernels_gemm_tall16.hip: f16_residual_kernel);
    // 0 = not measured (the per-element worst case 2^-11 stands in)
    DevBuf<uint32_t> d_xh_rho2;
    float xh_rho = 0.f;
    bool xh_exact = false;       // fp16 rows, image not centred: the image IS the rows (rho_x = 0, measured)
    bool xh_offset_dom = false;  // |c|^2 is several times the largest centred |x - c|^2: plain L2 keys cancel on this data, so
                                 // AUTO keeps batched searches on the centred image whatever the cost model says of other routes
    int64_t xh_declined_n = 0;   // a centred image was out of fp16's range at this many rows: not tried again below twice that
    // data whose neighbours the candidate keys cannot separate (tight clusters): batched searches start with the widened
    // candidate list that proved the last such batch, for the next kc_hint_left searches (search_batch_device)
    std::atomic<int> kc_hint{0}, kc_hint_left{0};

    Stream add_stream;
    PinnedBuf<char> h_stage[2]; // Add's staging slabs, taken by the first host Add
    EventH stage_ev[2];

    std::mutex ws_mu;
    std::vector<std::unique_ptr<Workspace>> ws_free;
    std::vector<std::unique_ptr<HostStage>> hs_free;

    SearchCombiner combiner; // concurrent host-pointer searches of a few queries each are combined (lb_host.h)

    std::atomic<int64_t> last_fallbacks{0};
    std::atomic<int> last_route{0}; // RouteKind * 10 + operand form of the most recent batched search (0: exact scan path)
    std::atomic<int64_t> fused_giveups{0}; // fused sample launches whose waits gave up (batch redone on the exact path)
    std::atomic<int> profiling{0};
    std::mutex prof_mu;
    float prof_ms[5] = {0, 0, 0, 0, 0};
    int prof_n[5] = {0, 0, 0, 0, 0};
    float refine_ms[3] = {0, 0, 0}; // the last profiled refine, summed over its batches: prepare, scan (with the query norms), selection

    size_t elem_bytes() const { return i8_rows ? 1 : f16_rows ? 2 : sizeof(float); }
    int dtype() const { return i8_rows ? 2 : f16_rows ? 1 : 0; } // simd.DataType
    const _Float16 *rows_f16() const { return reinterpret_cast<const _Float16 *>(d_X); }
    const int8_t *rows_i8() const { return reinterpret_cast<const int8_t *>(d_X); }
    // an int8 index keeps its exact int32 row norms (the sum of x_i^2 over i < 16 floor(D / 16)) in d_norm2's words
    int32_t *norm2_i8() const { return reinterpret_cast<int32_t *>(d_norm2.get()); }
};

// the handle's view, or (w: the call's workspace) the view of a call that brought its own bitmap
static IndexRowView row_view(const lb_gpu_index *h, const Workspace *w = nullptr)
{
    if (w && w->call_view) return w->cv;
    if (!h->has_mask) return {nullptr, nullptr, h->n};
    if (h->rowmap_on) return {nullptr, h->d_rowmap.get(), h->n_visible};
    return {h->d_mask.get(), nullptr, h->n};
}

// a sampled first pass (index_search.hip: sample_plan)
struct SamplePlan {
    bool on = false;
    int64_t span = 0;   // positions covered by the first pass
    uint32_t count = 0; // sampled rows
    int m = 0;
};

// f(X) with the index's rows typed as they are stored: f32, or fp16 on an fp16 index (the launchers overload on the row type;
// an int8 index's launchers take other arguments and are called apart)
template <class F> void with_rows(const lb_gpu_index *h, F &&f)
{
    if (h->f16_rows) f(h->rows_f16());
    else f(static_cast<const float *>(h->d_X));
}

// candidate-list geometry for a request of k (index_search.hip)
LB_INTERNAL void cand_geometry(int k, int &kc, uint32_t &cap);
// the index's workspace pool (index_search.hip)
LB_INTERNAL std::unique_ptr<Workspace> acquire_ws(lb_gpu_index *h, int nq, uint32_t cap);
LB_INTERNAL void release_ws(lb_gpu_index *h, std::unique_ptr<Workspace> w);
// index.hip, for index_remove.hip: the row list from d_mask, the accelerator images, and the flags finish_add derives from the
// norm statistics in d_maxnorm2 (the caller holds the exclusive lock)
LB_INTERNAL void rebuild_rowmap(lb_gpu_index *h);
LB_INTERNAL void drop_f16_image(lb_gpu_index *h);
LB_INTERNAL void drop_split_image(lb_gpu_index *h);
LB_INTERNAL void sync_split_image(lb_gpu_index *h);
LB_INTERNAL void sync_f16_image(lb_gpu_index *h);
LB_INTERNAL void set_norm_flags(lb_gpu_index *h, const uint32_t nbits[2]);
// call: the element type of the entry point (0 float32, 1 _f16, 2 _i8); LB_OK, or the error an index of another type reports (index.hip)
LB_INTERNAL int dtype_mismatch(lb_gpu_index *h, int call);
