// Host-only: one owned block of device (hipMalloc) or pinned host (hipHostMalloc) memory.
//
// Move-only; the destructor frees.  Converts to T * so that launch and copy sites read like a raw pointer.
// grow() is grow-only: nothing when the block is large enough, otherwise the old block is freed FIRST (the
// arenas are a large part of the device) and `need` elements are allocated; the contents are not kept.
//
// alloc_fill (acx_debug_set_alloc_fill, process-wide, off by default): while on, grow() fills every DEVICE block it allocates with
// one 32-bit word (bytes behind the last whole word: with its low byte) before anyone uses it, so that a test decides what a
// kernel finds in memory it never wrote.  Pinned host blocks are not filled.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace acx {

struct AllocFill { bool on = false; unsigned word = 0; };
inline AllocFill g_alloc_fill;

// `bytes` of device memory at p become `word` repeated; synchronous (hipMemsetD32 on the null stream, then the device is idle)
inline hipError_t fill_words(void *p, size_t bytes, unsigned word)
{
    hipError_t e = hipSuccess;
    if (bytes / 4) e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), (int)word, bytes / 4);
    if (e == hipSuccess && bytes % 4) e = hipMemset(static_cast<char *>(p) + bytes / 4 * 4, (int)(word & 0xffu), bytes % 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

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
        if (!PINNED && g_alloc_fill.on) return fill(g_alloc_fill.word);
        return hipSuccess;
    }
    // every byte of a device block, to capacity (debug exports only)
    hipError_t fill(unsigned word) const
    {
        return (PINNED || !p_) ? hipSuccess : fill_words(p_, cap_ * sizeof(T), word);
    }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

template <typename T>
using PinnedBuffer = DeviceBuffer<T, true>;

}  // namespace acx
