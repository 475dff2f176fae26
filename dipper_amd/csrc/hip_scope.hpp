// Scope owners for the HIP resources a host function creates for its own duration (host-only code).  Function-local HIP
// resources are owned by scope; only state that outlives a call is released by `*_free` / dpr_destroy.  Releasing does what the
// hand-written code did: one destroy call, its error ignored.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace dpr {

template <class Handle, hipError_t (*Destroy)(Handle)>
class HipOwner {
public:
    HipOwner() = default;
    HipOwner(HipOwner&& o) noexcept : h_(o.h_) { o.h_ = Handle{}; }      // (movable so that a std::vector can hold owners)
    HipOwner(const HipOwner&) = delete;
    HipOwner& operator=(const HipOwner&) = delete;
    ~HipOwner() { reset(); }
    void reset() { if (h_) (void)Destroy(h_); h_ = Handle{}; }
    Handle get() const { return h_; }
    operator Handle() const { return h_; }
    Handle* put() { reset(); return &h_; }   // for the create call: hipEventCreate(ev.put())

private:
    Handle h_{};
};

using ScopedEvent = HipOwner<hipEvent_t, hipEventDestroy>;
using ScopedGraph = HipOwner<hipGraph_t, hipGraphDestroy>;
using ScopedGraphExec = HipOwner<hipGraphExec_t, hipGraphExecDestroy>;
using ScopedStream = HipOwner<hipStream_t, hipStreamDestroy>;

template <class T> inline hipError_t hip_free_typed(T* p) { return hipFree((void*)p); }
// device memory of `count` elements of T: DPR_HIP(buf.alloc(count)); converts to T* for kernel arguments and copies
template <class T>
class DevBuf : public HipOwner<T*, hip_free_typed<T>> {
public:
    hipError_t alloc(size_t count) { return hipMalloc((void**)this->put(), count * sizeof(T)); }
};

}  // namespace dpr
