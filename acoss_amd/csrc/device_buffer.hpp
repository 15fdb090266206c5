// Host-only: one owned block of device (hipMalloc) or pinned host (hipHostMalloc) memory.
//
// Move-only; the destructor frees.  Converts to T * so that launch and copy sites read like a raw pointer.
// grow() is grow-only: nothing when the block is large enough, otherwise the old block is freed FIRST (the
// arenas are a large part of the device) and `need` elements are allocated; the contents are not kept.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace acx {

template <typename T, bool PINNED = false>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        if (this != &o) { (void)reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DeviceBuffer() { (void)reset(); }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }      // elements

    hipError_t reset()
    {
        T *p = p_;
        p_ = nullptr; cap_ = 0;
        if (!p) return hipSuccess;
        return PINNED ? hipHostFree(p) : hipFree(p);
    }
    // a failed allocation leaves the buffer empty and HIP's sticky error cleared
    hipError_t grow(size_t need)
    {
        if (need <= cap_) return hipSuccess;
        hipError_t e = reset();
        if (e != hipSuccess) return e;
        void *p = nullptr;
        e = PINNED ? hipHostMalloc(&p, need * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, need * sizeof(T));
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
        p_ = static_cast<T *>(p);
        cap_ = need;
        return hipSuccess;
    }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

template <typename T>
using PinnedBuffer = DeviceBuffer<T, true>;

}  // namespace acx
