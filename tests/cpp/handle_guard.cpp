// The shell of every entry point (longbow_amd/csrc/lb_handle.h: guard, guard_device) on a bare HandleCore, without a device:
// what a body returns or throws comes back as an lb_status and, on a handle, a last_error text; nothing else leaves.  The
// stream is null throughout, so no HIP call but the clearing of the last error is made.  tests/test_handle_guard.py builds
// and runs it.
#include "lb_handle.h"

#include <cstdio>
#include <cstring>

using namespace lb;

static int failures = 0;

static void expect(const char *what, int got, int want, const HandleCore *h, const char *text)
{
    const char *msg = h ? handle_last_error(h) : "";
    if (got == want && (!h || std::strcmp(msg, text) == 0)) return;
    std::printf("FAIL %s: status %d (want %d), last_error \"%s\" (want \"%s\")\n", what, got, want, msg, text);
    failures++;
}

// every body once inside guard() on a fresh handle and once inside guard_device()
template <class Body> static void both(const char *what, int want, const char *text, Body body)
{
    HandleCore h;
    expect(what, guard(&h, nullptr, body), want, &h, text);
    expect(what, guard_device(nullptr, body), want, nullptr, "");
}

int main()
{
    both("a status", LB_ERR_UNSUPPORTED, "", []() -> int { return LB_ERR_UNSUPPORTED; });
    both("ok", LB_OK, "", []() -> int { return LB_OK; });
    both("HipErr out of memory", LB_ERR_OOM, "HIP error 2 (out of memory) in hipMalloc (test)",
         []() -> int { throw HipErr{hipErrorOutOfMemory, "hipMalloc (test)"}; });
    both("HipErr invalid value", LB_ERR_HIP, "HIP error 1 (invalid argument) in hipMemcpy (test)",
         []() -> int { throw HipErr{hipErrorInvalidValue, "hipMemcpy (test)"}; });
    both("bad_alloc", LB_ERR_OOM, "out of host memory", []() -> int { throw std::bad_alloc(); });
    both("CtxErr cancelled", LB_ERR_CANCELLED, "context canceled", []() -> int { throw CtxErr{LB_ERR_CANCELLED}; });
    both("CtxErr deadline", LB_ERR_DEADLINE, "context deadline exceeded", []() -> int { throw CtxErr{LB_ERR_DEADLINE}; });
    both("an int", LB_ERR_INTERNAL, "internal error (exception)", []() -> int { throw 42; });
    {   // a later failure replaces the text; a success leaves it
        HandleCore h;
        (void)guard(&h, nullptr, []() -> int { throw CtxErr{LB_ERR_CANCELLED}; });
        (void)guard(&h, nullptr, []() -> int { throw std::bad_alloc(); });
        expect("second failure", guard(&h, nullptr, []() -> int { return LB_OK; }), LB_OK, &h, "out of host memory");
        expect("null handle", LB_OK, LB_OK, nullptr, "");
        if (std::strcmp(handle_last_error(nullptr), "null handle") != 0) { std::printf("FAIL null handle text\n"); failures++; }
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
