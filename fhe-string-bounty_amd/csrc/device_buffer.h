// device_buffer.h -- the one owner of device memory on the host side (engine.h, circuit.h), and HIP_TRY.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>

namespace fhe {

int fail(const std::string& msg);   // engine.hip: records the message for fhe_last_error, returns 1

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(std::string(#expr) + ": " + hipGetErrorString(_e));                   \
    } while (0)

// One hipMalloc allocation and its size.  hipFree synchronises the device, so a release is safe against work ordered on
// the freeing thread's streams; whoever releases a buffer that ANOTHER stream may still read waits for that stream first
// (Engine::reserve_idle).  The result of hipFree is ignored: there is nothing a caller could do about it.
template <class T>
struct DeviceBuffer {
    T* ptr = nullptr;
    size_t bytes = 0;

    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) { release(); ptr = o.ptr; bytes = o.bytes; o.ptr = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DeviceBuffer() { release(); }

    operator T*() const { return ptr; }   // kernel argument structs, copies, pointer arithmetic, "is it there"

    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr; bytes = 0;
    }
    // exactly n bytes, whatever was held before (a resident key being replaced); empty on failure
    int alloc(size_t n) {
        release();
        void* fresh = nullptr;
        HIP_TRY(hipMalloc(&fresh, n));
        ptr = static_cast<T*>(fresh); bytes = n;
        return 0;
    }
    // at least `need` bytes; contents are not kept when it has to grow; empty on failure
    int reserve(size_t need) { return bytes >= need ? 0 : alloc(need); }
};

}  // namespace fhe
