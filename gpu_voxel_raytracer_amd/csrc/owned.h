// owned.h — the owners of what the host code gets from the HIP runtime: device memory, pinned host memory, events and streams.
// Each is move-only, holds one handle (null: nothing), and gives it back in its destructor, which ignores the HIP status.  Each
// converts implicitly to the raw handle, so kernel launchers and HIP calls take an owner where they took the pointer.  Nothing is
// counted, pooled or logged.  The only calls that release a HIP resource in csrc/ are the four in this file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

namespace vxrt {

// hipMalloc / hipFree.  DeviceBuf<void> counts bytes and is read through as<T>().
template <typename T> class DeviceBuf {
    T* p_ = nullptr;
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(o.release()) {}
    DeviceBuf& operator=(DeviceBuf&& o) noexcept { if (this != &o) adopt(o.release()); return *this; }
    ~DeviceBuf() { reset(); }
    // `count` elements of fresh memory; what was held is released first.  On failure the buffer is empty.
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), count * sizeof(std::conditional_t<std::is_void_v<T>, char, T>));
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    void adopt(T* p) { reset(); p_ = p; }                    // p came from hipMalloc and has no other owner
    T* release() { return std::exchange(p_, nullptr); }      // the caller owns it from here
    void swap(DeviceBuf& o) noexcept { std::swap(p_, o.p_); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    template <typename U> U* as() const { return static_cast<U*>(p_); }
};

// hipHostMalloc / hipHostFree
template <typename T> class PinnedBuf {
    T* p_ = nullptr;
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); } return *this; }
    ~PinnedBuf() { reset(); }
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
};

class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); } return *this; }
    ~Event() { reset(); }
    hipError_t create(unsigned flags) {
        reset();
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    operator hipEvent_t() const { return e_; }
};

class Stream {
    hipStream_t s_ = nullptr;
    hipError_t made(hipError_t e) { if (e != hipSuccess) s_ = nullptr; return e; }
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s_ = std::exchange(o.s_, nullptr); } return *this; }
    ~Stream() { reset(); }
    hipError_t create(unsigned flags) { reset(); return made(hipStreamCreateWithFlags(&s_, flags)); }
    hipError_t create(unsigned flags, int priority) { reset(); return made(hipStreamCreateWithPriority(&s_, flags, priority)); }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    operator hipStream_t() const { return s_; }
};

}  // namespace vxrt
