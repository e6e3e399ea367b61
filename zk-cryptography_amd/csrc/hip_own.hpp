// hip_own.hpp -- owners of HIP resources: the only place in csrc/ that releases one.
// A deleter frees on whatever device is current: the object that holds owners makes its device current once, at the
// one place where its members go away (zkhip_ctx_destroy, zkhip_circuit_destroy, ...), not each deleter.
// A plain hipStream_t / hipEvent_t / void* next to an owner is a non-owning view of a handle owned elsewhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <initializer_list>
#include <memory>

#include "../../include/zkhip.h"

namespace zk {

struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct PinFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct GraphDestroy { void operator()(hipGraph_t g) const { (void)hipGraphDestroy(g); } };
struct GraphExecDestroy { void operator()(hipGraphExec_t g) const { (void)hipGraphExecDestroy(g); } };

using DevMem = std::unique_ptr<void, DevFree>;                          // hipMalloc
using PinMem = std::unique_ptr<void, PinFree>;                          // hipHostMalloc
using Event = std::unique_ptr<ihipEvent_t, EventDestroy>;
using Stream = std::unique_ptr<ihipStream_t, StreamDestroy>;
using Graph = std::unique_ptr<ihipGraph, GraphDestroy>;
using GraphExec = std::unique_ptr<hipGraphExec, GraphExecDestroy>;

// (re)allocate: the owner holds the new block, or nothing when the allocation failed
inline hipError_t dev_alloc(DevMem& m, size_t bytes) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    m.reset(e == hipSuccess ? p : nullptr);
    return e;
}
inline hipError_t pin_alloc(PinMem& m, size_t bytes, unsigned flags = hipHostMallocDefault) {
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, flags);
    m.reset(e == hipSuccess ? p : nullptr);
    return e;
}
// releases a block handed out raw through the C ABI (zkhip_malloc / zkhip_free)
inline hipError_t dev_free_raw(void* p) { return hipFree(p); }

// create on first use; an owner that already holds a handle is left alone
inline hipError_t ensure_event(Event& ev, unsigned flags = hipEventDisableTiming) {
    if (ev) return hipSuccess;
    hipEvent_t e = nullptr;
    const hipError_t rc = hipEventCreateWithFlags(&e, flags);
    if (rc == hipSuccess) ev.reset(e);
    return rc;
}
// non-blocking; without a priority it is created by hipStreamCreateWithFlags, as the side streams always were
inline hipError_t ensure_stream(Stream& st, const int* priority = nullptr) {
    if (st) return hipSuccess;
    hipStream_t s = nullptr;
    const hipError_t rc = priority ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, *priority) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (rc == hipSuccess) st.reset(s);
    return rc;
}
enum class Prio { Low, High };                                          // the ends of the device's priority range
inline hipError_t ensure_stream(Stream& st, Prio prio) {
    if (st) return hipSuccess;
    int least = 0, greatest = 0;
    const hipError_t rc = hipDeviceGetStreamPriorityRange(&least, &greatest);
    return rc != hipSuccess ? rc : ensure_stream(st, prio == Prio::Low ? &least : &greatest);
}

// Grow-only buffer, device (reserve) or pinned host memory (reserve_pinned; one kind per buffer).  A block that is large enough is
// kept; otherwise reserve waits for `drain` (the streams whose queued work may still touch the old block), frees the old block and
// allocates `want` bytes.  Rounding and floors are the caller's: it passes the size it wants to end up with.  Returns ZKHIP_OK,
// ZKHIP_ERR_HIP (a drain failed: the old block is kept) or ZKHIP_ERR_NOMEM (the buffer is empty then); *last_hip gets the error.
struct GrowBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    bool pinned = false;
    GrowBuf() = default;
    GrowBuf(const GrowBuf&) = delete;
    GrowBuf& operator=(const GrowBuf&) = delete;
    ~GrowBuf() { drop(); }
    void drop() {
        if (ptr) (void)(pinned ? hipHostFree(ptr) : hipFree(ptr));
        ptr = nullptr; bytes = 0;
    }
    int reserve_pinned(size_t want) { pinned = true; return reserve(want); }
    int reserve(size_t want, std::initializer_list<hipStream_t> drain = {}, int* last_hip = nullptr) {
        if (want <= bytes) return ZKHIP_OK;
        hipError_t e = hipSuccess;
        for (hipStream_t s : drain)
            if ((e = hipStreamSynchronize(s)) != hipSuccess) { if (last_hip) *last_hip = (int)e; return ZKHIP_ERR_HIP; }
        drop();
        e = pinned ? hipHostMalloc(&ptr, want, hipHostMallocDefault) : hipMalloc(&ptr, want);
        if (e != hipSuccess) { ptr = nullptr; if (last_hip) *last_hip = (int)e; return ZKHIP_ERR_NOMEM; }
        bytes = want;
        return ZKHIP_OK;
    }
};

}  // namespace zk
