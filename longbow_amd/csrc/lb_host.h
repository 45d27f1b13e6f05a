// lb_host.h -- host-side helpers shared by the C-ABI translation units (index.hip, index_search.hip, simd_api.hip, pq.hip,
// pq_train.hip, bq.hip, sq8.hip, comm.hip): HIP error plumbing, a pooled device / pinned-host buffer cache and the owners of a
// handle's own buffers.  lb_handle.h adds the shell every handle shares on top of it (the core of a handle, the guard an entry
// point runs in, the slab of a host-pointer search) and what the code-index handles (pq.hip, bq.hip, sq8.hip) share beyond that.
//
// Why a pool: hipMalloc costs 0.1-0.3 ms and hipFree synchronises the whole device, so an entry
// point that allocates per call stalls every concurrent search on the same GPU.  The host-pointer
// entry points (lb_simd_*, lb_gpu_index_filter_*, lb_gpu_rrf_fuse, lb_gpu_index_rerank, PQ) borrow
// their staging buffers from this cache instead.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <utility>
#include <vector>

#include "lb_combine.h"

namespace lb {

struct HipErr {
    hipError_t e;
    const char *what;
};

#define LB_HIP(call)                                          \
    do {                                                      \
        hipError_t _e = (call);                               \
        if (_e != hipSuccess) throw ::lb::HipErr{_e, #call};  \
    } while (0)

// A kernel launch with an illegal configuration (too much LDS, bad grid) is only reported by
// hipGetLastError; stream synchronisation returns success.  Every public entry point calls this
// once after its launches and before it reports LB_OK.
#define LB_LAUNCH_CHECK()                                                  \
    do {                                                                   \
        hipError_t _e = hipGetLastError();                                 \
        if (_e != hipSuccess) throw ::lb::HipErr{_e, "kernel launch"};     \
    } while (0)

// host-side types and functions shared between translation units that are no part of the library's ABI: kept out of its dynamic symbols
#define LB_INTERNAL __attribute__((visibility("hidden")))

class LB_INTERNAL BufPool {
  public:
    // device memory (pinned == false) on `device`, or pinned host memory; at least `bytes` long
    void *get(int device, size_t bytes, bool pinned)
    {
        if (bytes == 0) bytes = 1;
        {
            std::lock_guard<std::mutex> g(mu_);
            size_t best = (size_t)-1;
            for (size_t i = 0; i < free_.size(); i++) {
                const Ent &e = free_[i];
                if (e.device != device || e.pinned != pinned || e.bytes < bytes || e.bytes > 4 * bytes + (1u << 20)) continue;
                if (best == (size_t)-1 || e.bytes < free_[best].bytes) best = i;
            }
            if (best != (size_t)-1) {
                Ent e = free_[best];
                free_.erase(free_.begin() + (long)best);
                live_.push_back(e);
                return e.p;
            }
        }
        Ent e;
        e.device = device;
        e.pinned = pinned;
        e.bytes = (bytes + 65535) & ~(size_t)65535;
        e.p = nullptr;
        hipError_t rc = pinned ? hipHostMalloc(&e.p, e.bytes, hipHostMallocDefault) : hipMalloc(&e.p, e.bytes);
        if (rc != hipSuccess) {
            trim(device); // give cached buffers back and retry once
            rc = pinned ? hipHostMalloc(&e.p, e.bytes, hipHostMallocDefault) : hipMalloc(&e.p, e.bytes);
            if (rc != hipSuccess) throw HipErr{rc, pinned ? "hipHostMalloc (pool)" : "hipMalloc (pool)"};
        }
        std::lock_guard<std::mutex> g(mu_);
        live_.push_back(e);
        return e.p;
    }
    void put(void *p)
    {
        if (!p) return;
        Ent e{};
        bool drop = false;
        {
            std::lock_guard<std::mutex> g(mu_);
            size_t i = 0;
            for (; i < live_.size(); i++)
                if (live_[i].p == p) break;
            if (i == live_.size()) return; // not ours
            e = live_[i];
            live_.erase(live_.begin() + (long)i);
            size_t cached = 0, cached_bytes = 0;
            for (const Ent &f : free_)
                if (f.device == e.device && f.pinned == e.pinned) { cached++; cached_bytes += f.bytes; }
            // bounded cache: at most 16 buffers / 2 GiB per (device, kind)
            drop = cached >= 16 || cached_bytes + e.bytes > ((size_t)2 << 30);
            if (!drop) free_.push_back(e);
        }
        if (drop) {
            if (e.pinned) (void)hipHostFree(e.p);
            else (void)hipFree(e.p);
        }
    }
    // release every cached (not in use) buffer of `device` (-1: all devices)
    void trim(int device)
    {
        std::vector<Ent> out;
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t i = 0; i < free_.size();) {
                if (device < 0 || free_[i].device == device) {
                    out.push_back(free_[i]);
                    free_.erase(free_.begin() + (long)i);
                } else {
                    i++;
                }
            }
        }
        for (const Ent &e : out) {
            if (e.pinned) (void)hipHostFree(e.p);
            else (void)hipFree(e.p);
        }
    }

  private:
    struct Ent {
        int device;
        bool pinned;
        void *p;
        size_t bytes;
    };
    std::mutex mu_;
    std::vector<Ent> free_, live_;
};

BufPool &buf_pool(); // one per process (simd_api.hip)

// RAII lease from the pool
struct LB_INTERNAL Lease {
    void *p = nullptr;
    Lease() = default;
    Lease(int device, size_t bytes, bool pinned = false) : p(buf_pool().get(device, bytes, pinned)) {}
    Lease(const Lease &) = delete;
    Lease &operator=(const Lease &) = delete;
    ~Lease() { buf_pool().put(p); }
    void reset(int device, size_t bytes, bool pinned = false)
    {
        buf_pool().put(p);
        p = nullptr;
        p = buf_pool().get(device, bytes, pinned);
    }
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

// An array of T from hipMalloc (Pinned: hipHostMalloc), freed by the destructor; move-only.  A handle or a pooled scratch struct
// declares its buffers as members, and its own destructor only makes the device current: it runs before the members free
// themselves.
template <class T, bool Pinned> class LB_INTERNAL HipBuf {
  public:
    HipBuf() = default;
    HipBuf(HipBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    HipBuf &operator=(HipBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~HipBuf() { reset(); }
    T *get() const { return p_; }
    size_t count() const { return n_; } // elements allocated
    explicit operator bool() const { return p_ != nullptr; }
    void reset()
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    // exactly `count` elements, whatever was held before is freed first; throws HipErr and is then empty
    void alloc(size_t count)
    {
        reset();
        if (Pinned) LB_HIP(hipHostMalloc(&p_, count * sizeof(T), hipHostMallocDefault));
        else LB_HIP(hipMalloc(&p_, count * sizeof(T)));
        n_ = count;
    }
    // at least `count` elements; the contents are not kept when it has to re-allocate
    void ensure(size_t count) { if (n_ < count) alloc(count); }
    T *release() { n_ = 0; return std::exchange(p_, nullptr); }

  private:
    T *p_ = nullptr;
    size_t n_ = 0;
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinnedBuf = HipBuf<T, true>;

// a stream or an event, destroyed with its owner; created in place through `h`
template <class H, hipError_t (*Destroy)(H)> struct LB_INTERNAL HipHandle {
    H h = nullptr;
    HipHandle() = default;
    HipHandle(HipHandle &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    HipHandle &operator=(HipHandle &&) = delete;
    ~HipHandle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using Stream = HipHandle<hipStream_t, hipStreamDestroy>;
using EventH = HipHandle<hipEvent_t, hipEventDestroy>;

} // namespace lb

// context.Context's cancellation half for ONE call (include/longbow_gpu.h: lb_cancel_*).  The reference checks
// ctx.Err() every 1000 rows of its scan (internal/store/adaptive_index.go:182); here the host checks before every
// kernel launch of a search (a launch covers at most one pass over <= 2.5M rows / one PQ query), stops enqueuing,
// drains the stream and returns LB_ERR_CANCELLED / LB_ERR_DEADLINE.
struct lb_cancel {
    std::atomic<int> fired{0};
    std::atomic<long long> deadline_ns{0}; // steady clock; 0 = none
};

namespace lb {

struct CtxErr {
    int code;
};
inline int ctx_state(const lb_cancel *c)
{
    if (!c) return 0;
    if (c->fired.load(std::memory_order_relaxed)) return 8; // LB_ERR_CANCELLED
    const long long d = c->deadline_ns.load(std::memory_order_relaxed);
    if (d != 0 && std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() >= d)
        return 9; // LB_ERR_DEADLINE
    return 0;
}
inline void ctx_check(const lb_cancel *c)
{
    const int st = ctx_state(c);
    if (st) throw CtxErr{st};
}

inline bool device_ok(int device)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return false;
    return device >= 0 && device < cnt;
}

} // namespace lb
