// hip_owned.h -- the four things the host side allocates from the HIP runtime, each owned by exactly one object: a device block, a pinned
// host block, an event and a stream.  Non-copyable, movable, one creating call that returns the hipError_t, an implicit conversion to the raw
// pointer or handle (call sites read as with raw ones), release in the destructor.  The device the resource belongs to must be current when
// the owner dies (gg_destroy sets it before it deletes the context).  Nothing else: no registry, no sharing, no counting.
#pragma once

#include <hip/hip_runtime.h>

#include <utility>

namespace gg {

#pragma GCC visibility push(hidden) // internal to the library: none of this joins its exported symbols

// what the four share: the handle and how it moves.  `Owner` says how it is released.  An owner is created once, while it holds nothing:
// create() on one that holds a resource would overwrite the handle (every first-use site asks `if (!x)` first)
template <class Handle, class Owner> class HipOwned {
protected:
    Handle h = nullptr;
    hipError_t created(hipError_t e) // (a creating call that failed leaves nothing to release, whatever it wrote)
    {
        if (e != hipSuccess) h = nullptr;
        return e;
    }

public:
    HipOwned() = default;
    HipOwned(HipOwned &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    HipOwned &operator=(HipOwned &&o) noexcept { return std::swap(h, o.h), *this; } // (what this held dies with `o`)
    ~HipOwned()
    {
        if (h) Owner::release(h);
    }
    Handle get() const { return h; }
    operator Handle() const { return h; }
};

template <class T = void> struct DeviceBlock : HipOwned<T *, DeviceBlock<T>> {
    static void release(T *p) { (void)hipFree((void *)p); }
    hipError_t create(size_t bytes) { return this->created(hipMalloc((void **)&this->h, bytes)); }
};
template <class T = void> struct PinnedBlock : HipOwned<T *, PinnedBlock<T>> {
    static void release(T *p) { (void)hipHostFree((void *)p); }
    hipError_t create(size_t bytes, unsigned flags = hipHostMallocDefault) { return this->created(hipHostMalloc((void **)&this->h, bytes, flags)); }
};
struct Event : HipOwned<hipEvent_t, Event> {
    static void release(hipEvent_t e) { (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return created(hipEventCreateWithFlags(&h, flags)); }
};
struct Stream : HipOwned<hipStream_t, Stream> {
    static void release(hipStream_t s) { (void)hipStreamDestroy(s); }
    hipError_t create() { return created(hipStreamCreateWithFlags(&h, hipStreamNonBlocking)); }
};

#pragma GCC visibility pop

} // namespace gg
